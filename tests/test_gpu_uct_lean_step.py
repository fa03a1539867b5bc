"""uct_kernel's saturated form (uct_ldsr, csrc/uct.hip: THE LEAN TRIP): the terminal rule in the staged table, the record word
as 32 bits from its load on, one counter add per trip of two env steps, no carry compare in the generator's column 1.

The form stages the transition table whose bit 15 is the flag the model's rule stops on (csrc/uct_term_table.hpp: terminal[next]
with done_on_next, terminal[s] of the state a step leaves without it; tests/test_uct_lean_step_host.py pins both tables) and a
step tests that bit, in the descent and in the rollout.  None of it changes a result: every case compares EVERY root with the
oracle -- plans, plan lengths, root values, root children, env steps, generator records and the exported tree, node for node --
under both arms of the rollout's action table (MP_UCT_ACTION_TABLE=0 shares the step) and asserts the recorded kernel form.

  * both rules x |A| = 2..7 (7: the form without the action table) on 70 roots, one full wave and a tail of six lanes;
  * 2 x 1024 + 70 roots in workgroups of sixteen waves, one |A| per rule;
  * a chain of states that ends in a terminal one, a root at every distance from it: rollouts of every length from 1 to the
    horizon and beyond it (they end at the horizon exactly), so with the descents of five episodes rollouts that end in the
    trip's first step and in its second; a terminal root; a root whose first step ends the descent; the env's step limit with
    roots that have taken 0..3 steps of it.  The env steps of every root are asserted against the chain's arithmetic;
  * a model in which every terminal state leads to a live one and every other live state to a terminal one: the two tables
    differ in bit 15 of all but a few records, and the rules give different plans;
  * 20 000 states of two actions (next states with bit 14 set) and the largest model the form holds;
  * a kept tree continued for a second plan under the source rule (the first step of the second plan leaves the new root);
  * a model replaced whole and rewritten row by row, with and without new flags: both tables follow."""
import numpy as np
import pytest

from tests.helpers import assert_form, value_table

pytestmark = pytest.mark.gpu

KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_LONE_WAVES", "MP_UCT_EACH", "MP_UCT_ROW", "MP_UCT_ROWS",
         "MP_UCT_ROW_WAVES", "MP_UCT_ROW_ROOTS", "MP_UCT_PATH", "MP_UCT_LANES", "MP_UCT_LDSR_WAVES", "MP_UCT_POLICY_RECORD",
         "MP_UCT_COARSE_BITS", "MP_UCT_TREE_STORES", "MP_UCT_BALANCE", "MP_UCT_ACTION_TABLE", "MP_PIPE_CHUNK", "MP_PIPE_STREAMS")
ARMS = ("", "MP_UCT_ACTION_TABLE=0")
RULES = ("source", "next")
GAMMA, TEMPERATURE = 0.9, 5.0
EPISODES, HORIZON = 5, 6
TREE_FIELDS = ("parent", "action", "count", "value", "first_child")
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


def seeds(base, n):
    from rl_agents_amd import native
    return native.seed_sequence_states((), base, n)


def oracle_roots(t, r, term, rule, s0, rng0, k, steps0=None, max_steps=0, init_trees=None):
    from oracle import oracle
    p = np.ones(k) / k
    return [oracle.uct_plan(t, r, term, int(s0[i]), EPISODES, HORIZON, GAMMA, TEMPERATURE, p, p, rng0[i],
                            steps0=0 if steps0 is None else int(steps0[i]), max_steps=max_steps, done_rule=rule, max_plan_len=HORIZON,
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
        assert len(trees[i]["count"]) == len(ref["tree"]["count"]), w + ": tree size"
        for f in TREE_FIELDS:
            assert np.array_equal(trees[i][f], ref["tree"][f]), "{}: tree field {}".format(w, f)


def plan_once(ctx, model, s0, k, rng, root_steps=None):
    p = np.ones(k) / k
    out = ctx.uct_plan(model, s0, EPISODES, HORIZON, GAMMA, TEMPERATURE, p, p, rng, root_steps=root_steps, max_plan_len=HORIZON)
    assert_form(ctx, "uct_ldsr")       # (no case runs another kernel unnoticed)
    return out, rng.copy(), [ctx.uct_tree(i) for i in range(len(s0))]


def check_both_arms(ctx, monkeypatch, knobs, t, r, term, rule, s0, rng0, refs, what, root_steps=None, max_steps=0, table=None):
    """The plan under each arm of the action table, every root against ``refs``; ``table``: whether the default arm takes the
    action table (None: not asserted)."""
    k = t.shape[1]
    for arm in ARMS:
        set_knobs(monkeypatch, ("MP_UCT_MODEL=ldsr " + knobs + " " + arm).strip())
        model = ctx.load_table(t, r, term, done_rule=rule, max_steps=max_steps)
        _MODELS.append(model)
        ctx.uct_reset_tree()
        out, rng, trees = plan_once(ctx, model, s0, k, rng0.copy(), root_steps)
        if table is not None:
            assert ctx.uct_last_action_table() == (table and not arm)
        assert_against_oracle(out, rng, trees, refs, "{} / rule {} / {}".format(what, rule, arm or "default"))


def random_table(k, seed, n_states, terminal_rate):
    from rl_agents_amd.envs import generators
    cfg = generators.random_deterministic(n_states, k, seed, terminal_rate=terminal_rate)
    return cfg["transition"], cfg["reward"], cfg["terminal"]


# ---- both rules, every width: one full wave and a tail of six lanes ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("rule", RULES)
def test_rules_and_widths(ctx, monkeypatch, rule, k):
    n, n_states = 70, 23
    t, r, term = random_table(k, 900 + k, n_states, 0.15)
    assert term.any() and not term.all()
    s0 = (np.arange(n) * 5 % n_states).astype(np.int32)
    rng0 = seeds(41000 + 10 * k, n)
    refs = reference(("widths", rule, k), lambda: oracle_roots(t, r, term, rule, s0, rng0, k))
    check_both_arms(ctx, monkeypatch, "", t, r, term, rule, s0, rng0, refs, "|A| = {}".format(k), table=k <= 6)


# ---- a large batch in workgroups of sixteen waves ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,k", [("source", 5), ("next", 3)])
def test_large_batch_in_sixteen_wave_workgroups(ctx, monkeypatch, rule, k):
    n, n_states = 2 * 1024 + 70, 31
    t, r, term = random_table(k, 950 + k, n_states, 0.1)
    s0 = (np.arange(n) * 7 % n_states).astype(np.int32)
    rng0 = seeds(42000 + k, n)
    refs = reference(("large", rule, k), lambda: oracle_roots(t, r, term, rule, s0, rng0, k))
    check_both_arms(ctx, monkeypatch, "MP_UCT_LDSR_WAVES=16", t, r, term, rule, s0, rng0, refs, "large batch", table=True)


# ---- rollout endings: a chain that ends in a terminal state -----------------------------------------------------------------------------
CHAIN = 12


def chain(k):
    """State s leads to s + 1 under every action, the last state to itself and is terminal; rewards differ by action."""
    s, a = np.arange(CHAIN)[:, None], np.arange(k)[None, :]
    t = np.minimum(s + 1, CHAIN - 1) + 0 * a
    term = np.zeros(CHAIN, bool)
    term[CHAIN - 1] = True
    return t.astype(np.int64), ((s * 7 + a * 11) % 17) / 16.0, term


def chain_episode_steps(rule, s0, limit):
    """Env steps of EVERY episode from s0: the chain is the same under every action, so an episode -- descent and rollout
    together -- walks until its rule stops it, the horizon does or the env's step limit does (``limit`` steps left; the first
    step of an episode is unconditional)."""
    d = CHAIN - 1 - s0                                       # steps to ENTER the terminal state
    stop = max(d, 1) if rule == "next" else d + 1            # (source: the step that leaves the terminal state is the last)
    return max(1, min(stop, HORIZON, limit))


@pytest.mark.parametrize("rule", RULES)
def test_rollouts_of_every_length(ctx, monkeypatch, rule):
    k, n = 3, 70
    t, r, term = chain(k)
    s0 = (np.arange(n) % CHAIN).astype(np.int32)             # every distance 0..11 from the terminal state, the terminal root included
    rng0 = seeds(43000, n)
    refs = reference(("chain", rule), lambda: oracle_roots(t, r, term, rule, s0, rng0, k))
    want = [EPISODES * chain_episode_steps(rule, int(s), HORIZON) for s in s0]
    assert [ref["env_steps"] for ref in refs] == want
    per_episode = {w // EPISODES for w in want}
    assert per_episode == set(range(1, HORIZON + 1))         # length 1 .. the horizon exactly; odd and even; descents of depth 0..4 below
    check_both_arms(ctx, monkeypatch, "", t, r, term, rule, s0, rng0, refs, "chain", table=True)


@pytest.mark.parametrize("rule", RULES)
def test_the_step_limit_of_the_env(ctx, monkeypatch, rule):
    k, n, max_steps = 3, 70, 4
    t, r, term = chain(k)
    s0 = (np.arange(n) % CHAIN).astype(np.int32)
    steps0 = (np.arange(n) // CHAIN % max_steps).astype(np.int32)          # 0..3 steps of the limit taken: 4..1 left
    rng0 = seeds(43500, n)
    refs = reference(("limit", rule), lambda: oracle_roots(t, r, term, rule, s0, rng0, k, steps0=steps0, max_steps=max_steps))
    # the limit ends the rollouts of every root further than max_steps from the terminal state (a descent is not held to it, and a
    # rollout's first step is unconditional: no closed form here, the oracle counts)
    unlimited = [EPISODES * chain_episode_steps(rule, int(s), HORIZON) for s in s0]
    far = [CHAIN - 1 - int(s) > max_steps for s in s0]
    assert any(far) and all(ref["env_steps"] < w for ref, w, f in zip(refs, unlimited, far) if f)
    assert len({ref["env_steps"] for ref, f in zip(refs, far) if f}) >= max_steps       # (one count per number of steps left)
    check_both_arms(ctx, monkeypatch, "", t, r, term, rule, s0, rng0, refs, "step limit", root_steps=steps0, max_steps=max_steps, table=True)


# ---- terminal placement: what a swapped table bit would get wrong --------------------------------------------------------------------------
def swapped(k):
    """Eight states: 0 and 3 are terminal and lead to the live 1 and 2, which lead back to them; 4..7 are a live cycle that
    enters 0 from 7 under action 0 only."""
    t = np.zeros((8, k), np.int64)
    t[0], t[1], t[2], t[3] = 1, 0, 3, 2
    t[4], t[5], t[6], t[7] = 5, 6, 7, 4
    t[7, 0] = 0
    s, a = np.arange(8)[:, None], np.arange(k)[None, :]
    term = np.zeros(8, bool)
    term[[0, 3]] = True
    return t, ((s * 7 + a * 11) % 17) / 16.0, term


def test_terminal_states_with_live_successors_and_the_reverse(ctx, monkeypatch):
    k, n = 4, 70
    t, r, term = swapped(k)
    s0 = (np.arange(n) % 8).astype(np.int32)
    rng0 = seeds(44000, n)
    by_rule = {}
    for rule in RULES:
        by_rule[rule] = reference(("swapped", rule), lambda: oracle_roots(t, r, term, rule, s0, rng0, k))
        check_both_arms(ctx, monkeypatch, "", t, r, term, rule, s0, rng0, by_rule[rule], "swapped", table=True)
    # the rules are told apart: a terminal root stops after one step under "source" and walks on under "next", a live root next
    # to a terminal state the other way round
    for i in range(4):
        assert by_rule["source"][i]["env_steps"] != by_rule["next"][i]["env_steps"], i
    assert by_rule["source"][0]["env_steps"] == EPISODES and by_rule["next"][1]["env_steps"] == EPISODES


# ---- state width ------------------------------------------------------------------------------------------------------------------------
def wide_model(n_states):
    t, r, _ = value_table(n_states, 2)
    term = np.arange(n_states) % 7 == 3
    return t, r, term


def largest_ldsr_states(ctx, monkeypatch, n, k, n_rewards):
    """The largest S for which a plan of ``n`` roots takes the form under MP_UCT_MODEL=ldsr (mp_uct_choose_form: host only)."""
    from rl_agents_amd import native
    set_knobs(monkeypatch, "MP_UCT_MODEL=ldsr")

    def takes(s):
        try:
            name, _ = native.uct_choose_form([n, EPISODES, HORIZON, k, s, 1, s, 1, 1, n_rewards, 0, 0, -1, ctx.device_info()["n_cu"]])
        except native.NativeError:
            return False
        return name == "uct_ldsr"
    lo, hi = 20000, 32767
    assert takes(lo)
    if takes(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if takes(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("size", ["20000", "limit"])
def test_wide_states(ctx, monkeypatch, size, rule):
    k, n = 2, 70
    n_states = 20000 if size == "20000" else largest_ldsr_states(ctx, monkeypatch, n, k, 17)
    assert n_states >= 20000
    t, r, term = wide_model(n_states)
    s0 = (n_states - 1 - np.arange(n) * 3).astype(np.int32)                # roots and next states with bit 14 set
    assert (t[s0] >= 1 << 14).any() and s0.min() >= 1 << 14
    rng0 = seeds(45000, n)
    refs = reference(("wide", size, rule), lambda: oracle_roots(t, r, term, rule, s0, rng0, k))
    check_both_arms(ctx, monkeypatch, "", t, r, term, rule, s0, rng0, refs, "S = {}".format(n_states))


# ---- a kept tree continued under the source rule ------------------------------------------------------------------------------------------
def test_kept_tree_continued_under_the_source_rule(ctx, monkeypatch):
    from oracle import oracle
    k, n, n_states = 5, 70, 31
    t, r, term = random_table(k, 77, n_states, 0.2)
    s0 = (np.arange(n) * 3 % n_states).astype(np.int32)
    rng0 = seeds(46000, n)
    acts = (np.arange(n) % k).astype(np.int32)
    s1 = t[s0, acts].astype(np.int32)
    assert term[s1].any() and not term[s1].all()               # the second plan starts in terminal states and in live ones

    def on_the_host():
        plan1 = oracle_roots(t, r, term, "source", s0, rng0, k)
        kept = [oracle.uct_reroot(o["tree"], int(a), k) for o, a in zip(plan1, acts)]
        rng1 = np.stack([o["rng_after"] for o in plan1])
        return plan1, oracle_roots(t, r, term, "source", s1, rng1, k, init_trees=kept)
    plan1, plan2 = reference("kept", on_the_host)
    assert any(o["tree"]["first_child"][1 + a] >= 0 for o, a in zip(plan1, acts))      # subtrees are kept
    for arm in ARMS:
        set_knobs(monkeypatch, ("MP_UCT_MODEL=ldsr " + arm).strip())
        model = ctx.load_table(t, r, term, done_rule="source")
        _MODELS.append(model)
        ctx.uct_reset_tree()
        rng = rng0.copy()
        got1 = plan_once(ctx, model, s0, k, rng)
        assert_against_oracle(got1[0], got1[1], got1[2], plan1, "{} / first plan".format(arm or "default"))
        ctx.uct_step_tree(acts)
        got2 = plan_once(ctx, model, s1, k, rng)
        assert_against_oracle(got2[0], got2[1], got2[2], plan2, "{} / plan after the step".format(arm or "default"))
        ctx.uct_reset_tree()


# ---- both tables follow the model's updates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_tables_follow_model_updates(ctx, monkeypatch, rule):
    """A model replaced whole (update_tables), then three rows rewritten with their flags flipped and two without flags
    (update_rows): after each the plan is the oracle's on the tables as they then stand."""
    k, n, n_states = 5, 70, 23
    t0, r0, term0 = random_table(k, 61, n_states, 0.15)
    t, r, term = (x.copy() for x in random_table(k, 62, n_states, 0.3))
    s0 = (np.arange(n) * 5 % n_states).astype(np.int32)
    rng0 = seeds(47000, n)
    set_knobs(monkeypatch, "MP_UCT_MODEL=ldsr")
    model = ctx.load_table(t0, r0, term0, done_rule=rule)
    _MODELS.append(model)

    def check(what):
        refs = reference(("updates", rule, what), lambda: oracle_roots(t, r, term, rule, s0, rng0, k))
        ctx.uct_reset_tree()
        out, rng, trees = plan_once(ctx, model, s0, k, rng0.copy())
        assert_against_oracle(out, rng, trees, refs, "{} / rule {}".format(what, rule))
    model.update_tables(0, t[None], r[None], term[None])
    check("whole model replaced")
    rows = np.array([2, 9, 17], np.int32)
    t[rows] = (t[rows] + 3) % n_states
    r[rows] = r[rows][:, ::-1]
    term[rows] = ~term[rows]
    model.update_rows(rows, t[rows], r[rows], term[rows])
    check("rows with their flags flipped")
    rows = np.array([4, 11], np.int32)
    t[rows] = (t[rows] + 7) % n_states
    model.update_rows(rows, t[rows], r[rows])
    check("rows without flags")


def teardown_module(module):
    for m in _MODELS:
        m.close()
    del _MODELS[:]
