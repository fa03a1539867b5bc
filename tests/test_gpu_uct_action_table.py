"""uct_kernel's saturated form (uct_ldsr, csrc/uct.hip: ACTION TABLE) and the byte table its rollout reads its actions from.

With a state-independent policy a rollout step's action is a function of its draw, and for all but at most |A| - 1 of the 4 096
values of the draw's top twelve bits a function of those bits (csrc/uct_action_table.hpp; tests/test_uct_action_table_host.py pins
the table).  The kernel reads the byte of the draw's bucket and takes the exact compares, for the whole wave, only in a step where
some lane reads "a threshold lies in this bucket".  The table abbreviates the compares and nothing else, so the results are the
same BIT FOR BIT with MP_UCT_ACTION_TABLE=0, which launches the kernel without it: every case runs both arms, asserts the form and
the arm from the plan-call record (Context.last_kernel_variant, Context.uct_last_action_table) and compares each with the oracle
-- plans, plan lengths, root values, root children, env steps, generator records and the exported tree of EVERY root, node for node
-- and so with each other.

|A| in {2, 3, 5, 6, 8} (8: the kernel keeps the compares, the record says so) and a row of six actions with a zero in the middle
and trailing zeros; (episodes, horizon) = (5, 6); 2 x 64 + 6 roots (two full waves and a ragged one) and 70 roots in workgroups of
one wave and of four.  Two roots in three carry FORGED generator records (tests/forge.py) whose first, second or third rollout
draw is exactly a threshold, a threshold minus one, the first and the last value of the bucket that holds the threshold, the
first and the last value of a bucket that holds none, and 2^64 - 1; the third is seeded, so that in one wave the compares run for
everybody while other lanes hold table actions.  Then a kept tree continued, the same plan twice, and a model that leaves the
table's 4 096 bytes no room: the record says the table was not taken."""
import numpy as np
import pytest

from tests import forge
from tests.helpers import CDF_ROWS, assert_form, value_table

pytestmark = pytest.mark.gpu

KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_LONE_WAVES", "MP_UCT_EACH", "MP_UCT_ROW", "MP_UCT_ROWS",
         "MP_UCT_ROW_WAVES", "MP_UCT_ROW_ROOTS", "MP_UCT_PATH", "MP_UCT_LANES", "MP_UCT_LDSR_WAVES", "MP_UCT_POLICY_RECORD",
         "MP_UCT_COARSE_BITS", "MP_UCT_TREE_STORES", "MP_UCT_BALANCE", "MP_UCT_ACTION_TABLE", "MP_PIPE_CHUNK", "MP_PIPE_STREAMS")
ARMS = ("", "MP_UCT_ACTION_TABLE=0")
TABLE_ACTIONS = (2, 3, 4, 5, 6)              # uct_action_table_form: |A| = 7 and 8 keep the compares
GAMMA, TEMPERATURE = 0.9, 5.0
EPISODES, HORIZON = 5, 6
S = 12
BUCKET = 1 << 52                             # draws that share their top twelve bits
LDS_BYTES, BALANCE_BYTES, TABLE_BYTES = 160 * 1024, 64, 4096
TREE_FIELDS = ("parent", "action", "count", "value", "first_child")
OUT_FIELDS = ("plans", "plan_len", "env_steps", "root_value", "root_child_count", "root_child_value")
ROWS = {"uniform2": CDF_ROWS["uniform2"], "uniform3": CDF_ROWS["uniform3"], "uniform5": CDF_ROWS["uniform5"],
        "uniform6": np.ones(6) / 6, "uniform8": CDF_ROWS["uniform8"], "zeros": CDF_ROWS["zeros"]}
_REFS = {}
_MODELS = []


@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    yield c
    c.close()


def set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in knobs.split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv(k, v)


def reference(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def ctx_model(ctx, t, r, term, **kw):
    m = ctx.load_table(t, r, term, **kw)
    _MODELS.append(m)
    return m


# ---- forged records ------------------------------------------------------------------------------------------------------------------
def thresholds64(p):
    """The thresholds a rollout draw is compared with, on the raw 64-bit output: ceil(cdf[a] * 2^53) << 11 for a < |A| - 1, those
    of 2^53 (no draw reaches them) left out."""
    from oracle import oracle
    t53 = [forge.threshold53(c) for c in oracle.policy_cdf(p)[:-1]]
    return sorted({t << 11 for t in t53 if t < (1 << 53)})


def forged_draws(p):
    """64-bit outputs: every threshold, the threshold minus one, the first and the last value of the threshold's bucket; the first
    and the last value of two buckets that hold no threshold, the last one's last value being 2^64 - 1."""
    thr = thresholds64(p)
    out = []
    for t in thr:
        b = t >> 52
        out += [t, t - 1, b * BUCKET, b * BUCKET + BUCKET - 1]
    for b in (5, 4095):
        assert all(t >> 52 != b for t in thr)
        out += [b * BUCKET, b * BUCKET + BUCKET - 1]
    assert out[-1] == forge.M64
    return [d for d in dict.fromkeys(out) if 0 <= d <= forge.M64]


def mixed_records(p, n, skips, base):
    """``n`` records: root i with i % 3 == 2 seeded, the others forged -- for every skip of ``skips`` every draw of forged_draws as
    the (skip + 1)-th output, which is the (skip + 1)-th step of the plan's first rollout -- while there are draws left."""
    from rl_agents_amd import native
    rng = native.seed_sequence_states((), base, n)
    draws = [(d, skip) for skip in skips for d in forged_draws(p)]
    j = 0
    for i in range(n):
        if i % 3 == 2 or j == len(draws):
            continue
        d, skip = draws[j]
        j += 1
        rng[i] = forge.record((forge.DEFAULT_INC + 2 * i * 0x9E3779B97F4A7C15F39CC0605CEDC834) & forge.M128, d,
                              hi=(forge.DEFAULT_HI + i * 0x0400000000000001) & forge.M64,
                              buffered=0xC0FFEE00 + i if i & 1 else None, skip=skip)
    assert j == len(draws), "{} of {} forged draws found a root".format(j, len(draws))
    return rng


# ---- running and comparing -----------------------------------------------------------------------------------------------------------
def oracle_roots(t, r, term, s0, episodes, horizon, p, rng0, init_trees=None):
    from oracle import oracle
    prior = np.ones(len(p)) / len(p)                       # (the row under test is the ROLLOUT policy's)
    return [oracle.uct_plan(t, r, term, int(s0[i]), episodes, horizon, GAMMA, TEMPERATURE, prior, p, rng0[i], max_plan_len=horizon,
                            init_tree=None if init_trees is None else init_trees[i]) for i in range(len(s0))]


def assert_tree(got, want, what):
    assert len(got["count"]) == len(want["count"]), what + ": tree size"
    for f in TREE_FIELDS:
        assert np.array_equal(got[f], want[f]), "{}: tree field {}".format(what, f)


def assert_against_oracle(out, rng, trees, refs, what):
    for i, ref in enumerate(refs):
        w = "{}: root {}".format(what, i)
        assert out["plan_len"][i] == len(ref["plan"]), w
        np.testing.assert_array_equal(out["plans"][i, :len(ref["plan"])], ref["plan"], err_msg=w)
        assert out["env_steps"][i] == ref["env_steps"], w
        np.testing.assert_array_equal(rng[i], ref["rng_after"], err_msg=w)
        assert out["root_value"][i] == ref["tree"]["value"][0], w
        fc = ref["tree"]["first_child"][0]
        if fc >= 0:
            k = out["root_child_count"].shape[1]
            np.testing.assert_array_equal(out["root_child_count"][i], ref["tree"]["count"][fc:fc + k], err_msg=w)
            assert np.array_equal(out["root_child_value"][i], ref["tree"]["value"][fc:fc + k]), w
        assert_tree(trees[i], ref["tree"], w)


def assert_same_bytes(a, b, what):
    """two runs' outputs, generator records and trees, byte for byte"""
    for f in OUT_FIELDS:
        assert a[0][f].tobytes() == b[0][f].tobytes(), "{}: {}".format(what, f)
    assert a[1].tobytes() == b[1].tobytes(), what + ": generator records"
    assert len(a[2]) == len(b[2])
    for i, (x, y) in enumerate(zip(a[2], b[2])):
        for f in TREE_FIELDS:
            assert x[f].tobytes() == y[f].tobytes(), "{}: tree of root {}, field {}".format(what, i, f)


def assert_record(ctx, table):
    """the plan-call record: the form by name, and whether its action table was taken"""
    assert_form(ctx, "uct_ldsr")
    got = ctx.uct_last_action_table()
    assert got == table, "the action table was {} where the test means it {}".format("taken" if got else "not taken", "taken" if table else "left out")


def plan(ctx, t, r, term, s0, p, rng0, table):
    model = ctx_model(ctx, t, r, term)
    rng = rng0.copy()
    ctx.uct_reset_tree()
    out = ctx.uct_plan(model, s0, EPISODES, HORIZON, GAMMA, TEMPERATURE, np.ones(len(p)) / len(p), p, rng, max_plan_len=HORIZON)
    assert_record(ctx, table)
    return out, rng, [ctx.uct_tree(i) for i in range(len(s0))]


def both_arms(monkeypatch, knobs, run, fits=True):
    """``run(table)`` under each arm; ``table``: what the record must say of it"""
    got = []
    for arm in ARMS:
        set_knobs(monkeypatch, (knobs + " " + arm).strip())
        got.append(run(fits and not arm))
    return got


def random_table(k, seed, n_states, terminal_rate):
    from rl_agents_amd.envs import generators
    cfg = generators.random_deterministic(n_states, k, seed, terminal_rate=terminal_rate)
    return cfg["transition"], cfg["reward"], cfg["terminal"]


# ---- two full waves and a ragged one; forged first and third rollout draws on a table without terminal states --------------------------
@pytest.mark.parametrize("row", sorted(ROWS))
def test_two_full_waves_and_a_ragged_one(ctx, monkeypatch, row):
    p = ROWS[row]
    k, n = len(p), 2 * 64 + 6
    t, r, term = value_table(S, k)
    s0 = (np.arange(n) * 5 % S).astype(np.int32)
    rng0 = mixed_records(p, n, (0, 2), 31000 + 100 * k)
    refs = reference(("ragged", row), lambda: oracle_roots(t, r, term, s0, EPISODES, HORIZON, p, rng0))
    assert all(ref["env_steps"] == refs[0]["env_steps"] for ref in refs)      # (no rollout ends early: the forged draws are met)
    got = both_arms(monkeypatch, "MP_UCT_MODEL=ldsr", lambda table: plan(ctx, t, r, term, s0, p, rng0, table and k in TABLE_ACTIONS))
    for arm, (out, rng, trees) in zip(ARMS, got):
        assert_against_oracle(out, rng, trees, refs, arm or "default")
    assert_same_bytes(got[0], got[1], "default against MP_UCT_ACTION_TABLE=0")


# ---- 70 roots in workgroups of one wave and of four; forged second rollout draws; tables with terminal states -------------------------
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("row", sorted(ROWS))
def test_seventy_roots_in_small_workgroups(ctx, monkeypatch, row, waves):
    p = ROWS[row]
    k, n = len(p), 70
    t, r, term = random_table(k, 500 + k, 23, 0.1)
    s0 = (np.arange(n) * 5 % 23).astype(np.int32)
    rng0 = mixed_records(p, n, (1,), 32000 + 100 * k)
    refs = reference(("seventy", row), lambda: oracle_roots(t, r, term, s0, EPISODES, HORIZON, p, rng0))
    got = both_arms(monkeypatch, "MP_UCT_MODEL=ldsr MP_UCT_LDSR_WAVES={}".format(waves),
                    lambda table: plan(ctx, t, r, term, s0, p, rng0, table and k in TABLE_ACTIONS))
    for arm, (out, rng, trees) in zip(ARMS, got):
        assert_against_oracle(out, rng, trees, refs, "{} waves / {}".format(waves, arm or "default"))
    assert_same_bytes(got[0], got[1], "default against MP_UCT_ACTION_TABLE=0")


# ---- a kept tree continued (step_strategy "subtree") --------------------------------------------------------------------------------
def test_kept_tree_continued(ctx, monkeypatch):
    from oracle import oracle
    p = ROWS["uniform5"]
    k, n = 5, 2 * 64 + 6
    t, r, term = random_table(k, 77, 31, 0.05)
    s0 = (np.arange(n) * 3 % 31).astype(np.int32)
    rng0 = mixed_records(p, n, (0, 2), 33000)
    acts = (np.arange(n) % k).astype(np.int32)

    def on_the_host():
        plan1 = oracle_roots(t, r, term, s0, EPISODES, HORIZON, p, rng0)
        kept = [oracle.uct_reroot(o["tree"], int(a), k) for o, a in zip(plan1, acts)]
        s1 = t[s0, acts].astype(np.int32)
        rng1 = np.stack([o["rng_after"] for o in plan1])
        return plan1, s1, oracle_roots(t, r, term, s1, EPISODES, HORIZON, p, rng1, init_trees=kept)
    plan1, s1, plan2 = reference("kept", on_the_host)
    assert any(o["tree"]["first_child"][1 + a] >= 0 for o, a in zip(plan1, acts))      # subtrees are kept

    def run(table):
        model = ctx_model(ctx, t, r, term)
        rng = rng0.copy()
        ctx.uct_reset_tree()
        out1 = ctx.uct_plan(model, s0, EPISODES, HORIZON, GAMMA, TEMPERATURE, np.ones(len(p)) / len(p), p, rng, max_plan_len=HORIZON)
        assert_record(ctx, table)
        got1 = (out1, rng.copy(), [ctx.uct_tree(i) for i in range(n)])
        ctx.uct_step_tree(acts)
        out2 = ctx.uct_plan(model, s1, EPISODES, HORIZON, GAMMA, TEMPERATURE, np.ones(len(p)) / len(p), p, rng, max_plan_len=HORIZON)
        assert_record(ctx, table)
        got2 = (out2, rng.copy(), [ctx.uct_tree(i) for i in range(n)])
        ctx.uct_reset_tree()
        return got1, got2
    got = both_arms(monkeypatch, "MP_UCT_MODEL=ldsr", run)
    for arm, (got1, got2) in zip(ARMS, got):
        assert_against_oracle(got1[0], got1[1], got1[2], plan1, "{} / first plan".format(arm or "default"))
        assert_against_oracle(got2[0], got2[1], got2[2], plan2, "{} / plan after the step".format(arm or "default"))
    assert_same_bytes(got[0][1], got[1][1], "plan after the step: default against MP_UCT_ACTION_TABLE=0")


# ---- the same plan twice --------------------------------------------------------------------------------------------------------------
def test_the_same_plan_twice_gives_the_same_bytes(ctx, monkeypatch):
    p = ROWS["uniform5"]
    k, n = 5, 2 * 64 + 6
    t, r, term = random_table(k, 300 + k, 40, 0.1)
    s0 = (np.arange(n) * 5 % 40).astype(np.int32)
    rng0 = mixed_records(p, n, (0, 2), 34000)
    set_knobs(monkeypatch, "MP_UCT_MODEL=ldsr")
    first = plan(ctx, t, r, term, s0, p, rng0, True)
    second = plan(ctx, t, r, term, s0, p, rng0, True)
    assert_same_bytes(first, second, "the same plan twice")


# ---- a model that leaves the table no room ---------------------------------------------------------------------------------------------
def test_a_model_that_leaves_no_room_runs_without_the_table(ctx, monkeypatch):
    from rl_agents_amd import native
    p = ROWS["uniform5"]
    k, n, n_states = 5, 70, 10700
    t, r, term = value_table(n_states, k)
    set_knobs(monkeypatch, "MP_UCT_MODEL=ldsr")
    name, geo = native.uct_choose_form([n, EPISODES, HORIZON, k, n_states, 1, n_states, 1, 1, len(np.unique(r)), 0, 0, -1,
                                        ctx.device_info()["n_cu"]])
    lds = int(geo[native.UCT_FORM_FIELDS.index("lds")])
    assert name == "uct_ldsr" and lds + BALANCE_BYTES <= LDS_BYTES < lds + BALANCE_BYTES + TABLE_BYTES, (name, lds)
    s0 = (np.arange(n) * 151 % n_states).astype(np.int32)
    rng0 = mixed_records(p, n, (1,), 35000)
    refs = reference("no room", lambda: oracle_roots(t, r, term, s0, EPISODES, HORIZON, p, rng0))
    got = both_arms(monkeypatch, "MP_UCT_MODEL=ldsr", lambda table: plan(ctx, t, r, term, s0, p, rng0, table), fits=False)
    for arm, (out, rng, trees) in zip(ARMS, got):
        assert_against_oracle(out, rng, trees, refs, arm or "default")
    assert_same_bytes(got[0], got[1], "default against MP_UCT_ACTION_TABLE=0")


def teardown_module(module):
    for m in _MODELS:
        m.close()
    del _MODELS[:]
