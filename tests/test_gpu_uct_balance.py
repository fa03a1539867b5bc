"""uct_kernel's saturated form (uct_ldsr, csrc/uct.hip: WAVE BALANCE) and the priority of its rollouts.

Every wave of a workgroup keeps a progress word in LDS and runs its rollout at priority 1 while it has a mate on its SIMD and none
of them is in an earlier episode, at 0 otherwise (csrc/uct_balance.hpp; tests/test_uct_balance_rule_host.py pins the rule).  The
words decide a priority and nothing else, so the results are the same BIT FOR BIT with MP_UCT_BALANCE=0, which runs the kernel
without the words: every case runs both arms and compares each with the oracle -- plans, plan lengths, root values, root children,
env steps, generator records and the exported tree of EVERY root, node for node -- and so with each other.

Tables of 6 to 40 states, |A| in {2, 3, 5, 6}, (episodes, horizon) (33, 30) and (5, 3); 2 x 1024 + 70 roots in workgroups of
sixteen waves (the last one: a full wave, a tail wave of six lanes and fourteen waves that leave at entry), 70 roots in workgroups of
one wave (no mates) and of four, a launch whose first wave finishes every episode at once while its mates roll the full horizon, a
kept tree continued, and the same plan twice."""
import numpy as np
import pytest

from tests.helpers import assert_form

pytestmark = pytest.mark.gpu

KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_LONE_WAVES", "MP_UCT_EACH", "MP_UCT_ROW", "MP_UCT_ROWS",
         "MP_UCT_ROW_WAVES", "MP_UCT_ROW_ROOTS", "MP_UCT_PATH", "MP_UCT_LANES", "MP_UCT_LDSR_WAVES", "MP_UCT_POLICY_RECORD",
         "MP_UCT_COARSE_BITS", "MP_UCT_TREE_STORES", "MP_UCT_BALANCE", "MP_PIPE_CHUNK", "MP_PIPE_STREAMS")
ARMS = ("", "MP_UCT_BALANCE=0")
GAMMA, TEMPERATURE = 0.9, 5.0
TREE_FIELDS = ("parent", "action", "count", "value", "first_child")
OUT_FIELDS = ("plans", "plan_len", "env_steps", "root_value", "root_child_count", "root_child_value")
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


def records(n, base):
    from rl_agents_amd import native
    return native.seed_sequence_states((), base, n)


def table(k, seed, n_states, terminal_rate):
    from rl_agents_amd.envs import generators
    cfg = generators.random_deterministic(n_states, k, seed, terminal_rate=terminal_rate)
    return cfg["transition"], cfg["reward"], cfg["terminal"]


def ctx_model(ctx, t, r, term, **kw):
    m = ctx.load_table(t, r, term, **kw)
    _MODELS.append(m)
    return m


def oracle_roots(t, r, term, s0, episodes, horizon, p, rng0, mpl, init_trees=None):
    from oracle import oracle
    return [oracle.uct_plan(t, r, term, int(s0[i]), episodes, horizon, GAMMA, TEMPERATURE, p, p, rng0[i], max_plan_len=mpl,
                            init_tree=None if init_trees is None else init_trees[i]) for i in range(len(s0))]


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


def assert_tree(got, want, what):
    assert len(got["count"]) == len(want["count"]), what + ": tree size"
    for f in TREE_FIELDS:
        assert np.array_equal(got[f], want[f]), "{}: tree field {}".format(what, f)


def assert_same_bytes(a, b, what):
    """two runs' outputs, generator records and trees, byte for byte"""
    for f in OUT_FIELDS:
        assert a[0][f].tobytes() == b[0][f].tobytes(), "{}: {}".format(what, f)
    assert a[1].tobytes() == b[1].tobytes(), what + ": generator records"
    assert len(a[2]) == len(b[2])
    for i, (x, y) in enumerate(zip(a[2], b[2])):
        for f in TREE_FIELDS:
            assert x[f].tobytes() == y[f].tobytes(), "{}: tree of root {}, field {}".format(what, i, f)


def plan(ctx, t, r, term, s0, episodes, horizon, p, rng0):
    model = ctx_model(ctx, t, r, term)
    rng = rng0.copy()
    ctx.uct_reset_tree()
    out = ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
    assert_form(ctx, "uct_ldsr")
    return out, rng, [ctx.uct_tree(i) for i in range(len(s0))]


def both_arms(ctx, monkeypatch, knobs, run):
    got = []
    for arm in ARMS:
        set_knobs(monkeypatch, (knobs + " " + arm).strip())
        got.append(run())
    return got


# (|A|, episodes, horizon, states, terminal rate)
SHAPES = [(5, 33, 30, 40, 0.1), (2, 5, 3, 6, 0.0), (3, 33, 30, 17, 0.05), (6, 5, 3, 25, 0.1), (6, 33, 30, 31, 0.0), (2, 33, 30, 9, 0.0)]
SHAPE_IDS = ["A{}-E{}-H{}-S{}".format(*c[:4]) for c in SHAPES]


# ---- sixteen waves per workgroup: full workgroups, and one with a full wave, a tail wave and fourteen that leave at entry ----------
@pytest.mark.parametrize("case", SHAPES[:4], ids=SHAPE_IDS[:4])
def test_sixteen_waves_full_and_ragged_workgroups(ctx, monkeypatch, case):
    k, episodes, horizon, n_states, rate = case
    n = 2 * 1024 + 70
    t, r, term = table(k, 300 + k + episodes, n_states, rate)
    s0 = (np.arange(n) * 5 % n_states).astype(np.int32)
    rng0 = records(n, 21000 + 100 * k + episodes)
    p = np.ones(k) / k
    refs = reference(("sixteen", case), lambda: oracle_roots(t, r, term, s0, episodes, horizon, p, rng0, horizon))
    got = both_arms(ctx, monkeypatch, "MP_UCT_MODEL=ldsr MP_UCT_LDSR_WAVES=16", lambda: plan(ctx, t, r, term, s0, episodes, horizon, p, rng0))
    for arm, (out, rng, trees) in zip(ARMS, got):
        assert_against_oracle(out, rng, trees, refs, arm or "default")
    assert_same_bytes(got[0], got[1], "default against MP_UCT_BALANCE=0")


# ---- 70 roots: one wave per workgroup (no mates: the balance does nothing) and four ---------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("case", SHAPES, ids=SHAPE_IDS)
def test_seventy_roots_in_small_workgroups(ctx, monkeypatch, case, waves):
    k, episodes, horizon, n_states, rate = case
    n = 70
    t, r, term = table(k, 400 + k + episodes, n_states, rate)
    s0 = (np.arange(n) * 5 % n_states).astype(np.int32)
    rng0 = records(n, 22000 + 100 * k + episodes)
    p = np.ones(k) / k
    refs = reference(("seventy", case), lambda: oracle_roots(t, r, term, s0, episodes, horizon, p, rng0, horizon))
    got = both_arms(ctx, monkeypatch, "MP_UCT_MODEL=ldsr MP_UCT_LDSR_WAVES={}".format(waves),
                    lambda: plan(ctx, t, r, term, s0, episodes, horizon, p, rng0))
    for arm, (out, rng, trees) in zip(ARMS, got):
        assert_against_oracle(out, rng, trees, refs, "{} waves / {}".format(waves, arm or "default"))
    assert_same_bytes(got[0], got[1], "default against MP_UCT_BALANCE=0")


# ---- mates that really are episodes apart ------------------------------------------------------------------------------------------
def short_first_wave_table(k, n_states):
    """a random table in which state 0 leads to the terminal state n - 1 under every action and no other state leads to either:
    an episode from state 0 is one step long, an episode from any other state never ends before the horizon"""
    t, r, term = table(k, 91, n_states, 0.0)
    t = np.where((t == 0) | (t == n_states - 1), 1 + (t + np.arange(n_states)[:, None]) % (n_states - 2), t)
    t[0, :] = n_states - 1
    term = np.zeros(n_states, bool)
    term[n_states - 1] = True
    return t, r, term


@pytest.mark.parametrize("k", [5, 3])
def test_first_wave_one_step_from_the_end_its_mates_at_full_horizon(ctx, monkeypatch, k):
    episodes, horizon, n_states = 33, 30, 23
    n = 1024 + 70
    t, r, term = short_first_wave_table(k, n_states)
    s0 = (1 + np.arange(n) * 5 % (n_states - 2)).astype(np.int32)
    s0[:64] = 0                                                # the first wave of the first workgroup
    rng0 = records(n, 23000 + k)
    p = np.ones(k) / k
    refs = reference(("apart", k), lambda: oracle_roots(t, r, term, s0, episodes, horizon, p, rng0, horizon))
    steps = np.array([ref["env_steps"] for ref in refs])
    assert steps[:64].max() <= 2 * episodes                    # the step into the terminal state and the one that finds it so
    assert steps[64:].min() >= episodes * (horizon - 2)        # the others: (nearly) the full horizon in every episode
    got = both_arms(ctx, monkeypatch, "MP_UCT_MODEL=ldsr MP_UCT_LDSR_WAVES=16", lambda: plan(ctx, t, r, term, s0, episodes, horizon, p, rng0))
    for arm, (out, rng, trees) in zip(ARMS, got):
        assert_against_oracle(out, rng, trees, refs, arm or "default")
    assert_same_bytes(got[0], got[1], "default against MP_UCT_BALANCE=0")


# ---- a kept tree continued (step_strategy "subtree") --------------------------------------------------------------------------------
def test_kept_tree_continued(ctx, monkeypatch):
    from oracle import oracle
    k, episodes, horizon, n_states, n = 5, 9, 5, 31, 1024 + 70
    t, r, term = table(k, 77, n_states, 0.05)
    s0 = (np.arange(n) * 3 % n_states).astype(np.int32)
    rng0 = records(n, 24000)
    p = np.ones(k) / k
    acts = (np.arange(n) % k).astype(np.int32)

    def on_the_host():
        plan1 = oracle_roots(t, r, term, s0, episodes, horizon, p, rng0, horizon)
        kept = [oracle.uct_reroot(o["tree"], int(a), k) for o, a in zip(plan1, acts)]
        s1 = t[s0, acts].astype(np.int32)
        rng1 = np.stack([o["rng_after"] for o in plan1])
        return plan1, s1, oracle_roots(t, r, term, s1, episodes, horizon, p, rng1, horizon, init_trees=kept)
    plan1, s1, plan2 = reference("kept", on_the_host)
    assert any(o["tree"]["first_child"][1 + a] >= 0 for o, a in zip(plan1, acts))      # subtrees are kept

    def run():
        model = ctx_model(ctx, t, r, term)
        rng = rng0.copy()
        ctx.uct_reset_tree()
        out1 = ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
        assert_form(ctx, "uct_ldsr")
        got1 = (out1, rng.copy(), [ctx.uct_tree(i) for i in range(n)])
        ctx.uct_step_tree(acts)
        out2 = ctx.uct_plan(model, s1, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
        assert_form(ctx, "uct_ldsr")
        got2 = (out2, rng.copy(), [ctx.uct_tree(i) for i in range(n)])
        ctx.uct_reset_tree()
        return got1, got2
    got = both_arms(ctx, monkeypatch, "MP_UCT_MODEL=ldsr MP_UCT_LDSR_WAVES=16", run)
    for arm, (got1, got2) in zip(ARMS, got):
        assert_against_oracle(got1[0], got1[1], got1[2], plan1, "{} / first plan".format(arm or "default"))
        assert_against_oracle(got2[0], got2[1], got2[2], plan2, "{} / plan after the step".format(arm or "default"))
    assert_same_bytes(got[0][1], got[1][1], "plan after the step: default against MP_UCT_BALANCE=0")


# ---- the same plan twice --------------------------------------------------------------------------------------------------------------
def test_the_same_plan_twice_gives_the_same_bytes(ctx, monkeypatch):
    k, episodes, horizon, n_states, n = 5, 33, 30, 40, 2 * 1024 + 70
    t, r, term = table(k, 300 + k + episodes, n_states, 0.1)
    s0 = (np.arange(n) * 5 % n_states).astype(np.int32)
    rng0 = records(n, 25000)
    p = np.ones(k) / k
    set_knobs(monkeypatch, "MP_UCT_MODEL=ldsr MP_UCT_LDSR_WAVES=16")
    first = plan(ctx, t, r, term, s0, episodes, horizon, p, rng0)
    second = plan(ctx, t, r, term, s0, episodes, horizon, p, rng0)
    assert_same_bytes(first, second, "the same plan twice")


def teardown_module(module):
    for m in _MODELS:
        m.close()
    del _MODELS[:]
