"""uct_kernel (csrc/uct.hip) and the visited mask of its fresh trees: only the children an episode picked are stored or loaded.

A child that no episode has picked is {0.0, 0, -1} (csrc/uct_virgin.hpp; the count-1 rule of tests/test_uct_virgin_rule.py is
the special case of a parent whose children are all unpicked).  The default form of uct_ldsr, uct_global and uct_global_spill
(|A| <= 5) keeps, in the bits above 24 of an expanded node's first_child, which of its children were stored: a descent loads
those and takes the constant for the others, a first pick sets its bit, and no sibling is ever stored for its own sake.  The plan
read-out, the export, the re-rooting and mp_uct_path_count read the trees by the rule; re-rooted trees are whole again and their
words plain.  MP_UCT_TREE_STORES=virgin runs the count-1 rule with its sibling stores, =group every group stored and loaded.  The
results are the same BIT FOR BIT: every case runs the three arms and compares each with the oracle -- plans, plan lengths, root
values, root children, env steps, generator records and the exported tree of EVERY root, node for node.

70 roots (a full wave and a tail wave of six lanes) on tables of 6 to 40 states; |A| = 6 keeps its complete trees and runs as the
control.  Before each run a larger plan on another table fills the tree workspace with visited nodes (poison), so a node that is
read without the rule does not read as zeros by luck."""
import numpy as np
import pytest

from tests.helpers import assert_form

pytestmark = pytest.mark.gpu

KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_LONE_WAVES", "MP_UCT_EACH", "MP_UCT_ROW", "MP_UCT_ROWS",
         "MP_UCT_ROW_WAVES", "MP_UCT_ROW_ROOTS", "MP_UCT_PATH", "MP_UCT_LANES", "MP_UCT_LDSR_WAVES", "MP_UCT_POLICY_RECORD",
         "MP_UCT_COARSE_BITS", "MP_UCT_TREE_STORES", "MP_PIPE_CHUNK", "MP_PIPE_STREAMS")
FORMS = [("uct_ldsr", "MP_UCT_MODEL=ldsr"), ("uct_global", "MP_UCT_MODEL=global"),
         ("uct_global_spill", "MP_UCT_MODEL=global MP_UCT_PATH=spill")]
ARMS = ("", "MP_UCT_TREE_STORES=virgin", "MP_UCT_TREE_STORES=group")
N = 70
GAMMA, TEMPERATURE = 0.9, 5.0
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


def records(n, base):
    from rl_agents_amd import native
    return native.seed_sequence_states((), base, n)


def table(k, seed, n_states, terminal_rate):
    from rl_agents_amd.envs import generators
    cfg = generators.random_deterministic(n_states, k, seed, terminal_rate=terminal_rate)
    return cfg["transition"], cfg["reward"], cfg["terminal"]


def corridor(n_states, k):
    """state s moves to s + 1 under every action (the last state stays); action 0 pays most, so the search digs one deep path"""
    t = np.minimum(np.arange(n_states)[:, None] + 1, n_states - 1).repeat(k, axis=1).astype(np.int64)
    r = np.tile(np.linspace(1.0, 0.0, k), (n_states, 1))
    return t, r, np.zeros(n_states, np.uint8)


def ctx_model(ctx, t, r, term, **kw):
    m = ctx.load_table(t, r, term, **kw)
    _MODELS.append(m)
    return m


def poison(ctx, monkeypatch, knobs):
    """a plan whose trees are larger than any case's and hold no zero node in the slots the cases leave unstored: every node of
    a 3-state cycle with reward 1 is visited often, and the next plan on this ctx reuses the workspace.  It runs with
    MP_UCT_TREE_STORES=group, which stores every group of its own trees."""
    set_knobs(monkeypatch, (knobs + " MP_UCT_TREE_STORES=group").strip())
    t = np.array([[1, 2], [2, 0], [0, 1]], np.int64)
    r = np.ones((3, 2))
    p = np.ones(2) / 2
    rng = records(1100, 1)
    ctx.uct_reset_tree()
    ctx.uct_plan(ctx_model(ctx, t, r, None), np.zeros(1100, np.int32), 400, 12, GAMMA, 0.1, p, p, rng, max_plan_len=1)


def oracle_roots(t, r, term, s0, steps0, episodes, horizon, p, rng0, done_rule, max_steps, mpl, temperature=TEMPERATURE):
    """the oracle's plan and tree of every root -> list of dicts"""
    from oracle import oracle
    return [oracle.uct_plan(t, r, term, int(s0[i]), episodes, horizon, GAMMA, temperature, p, p, rng0[i], steps0=int(steps0[i]),
                            max_steps=max_steps, done_rule=done_rule, max_plan_len=mpl) for i in range(len(s0))]


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


def depths(tree, k):
    fc, depth = tree["first_child"], np.zeros(len(tree["count"]), int)
    for node in range(len(fc)):
        if fc[node] >= 0:
            depth[fc[node]:fc[node] + k] = depth[node] + 1
    return depth


def partly_visited(tree, k):
    """parents below the root that were entered at least twice and still hold a child nobody picked: their groups are read with
    some bits set and some clear"""
    cnt, fc = tree["count"], tree["first_child"]
    return [int(n) for n in np.flatnonzero((cnt >= 3) & (fc >= 0))[1:]
            if (cnt[fc[n]:fc[n] + k] == 0).any() and (cnt[fc[n]:fc[n] + k] > 0).any()]


def run_arms(ctx, monkeypatch, expect, knobs, run):
    got = []
    for arm in ARMS:
        poison(ctx, monkeypatch, knobs)
        set_knobs(monkeypatch, (knobs + " " + arm).strip())
        got.append(run(expect))
    return got


def plan_and_export(ctx, expect, model, s0, episodes, horizon, p, rng0, steps0=None, temperature=TEMPERATURE):
    rng = rng0.copy()
    ctx.uct_reset_tree()
    out = ctx.uct_plan(model, s0, episodes, horizon, GAMMA, temperature, p, p, rng, root_steps=steps0, max_plan_len=horizon)
    assert_form(ctx, expect)
    return out, rng, [ctx.uct_tree(i) for i in range(len(s0))]


# ---- fresh trees --------------------------------------------------------------------------------------------------------------
# (|A|, episodes, horizon, states, terminal rate, done rule, max_steps): |A| = 2..5 with the mask and |A| = 6 without (the
# control: the form keeps its complete trees), one and two episodes (no group below the root is entered), terminal states under
# both done rules, and a step limit that roots reach at different depths because they start at different step counts
FRESH = [(2, 33, 8, 40, 0.3, "next", 0), (3, 33, 6, 17, 0.1, "source", 0), (4, 33, 7, 21, 0.2, "next", 0),
         (5, 33, 30, 40, 0.1, "source", 0), (6, 33, 6, 30, 0.1, "source", 0), (5, 1, 4, 12, 0.0, "source", 0),
         (5, 2, 4, 12, 0.0, "source", 0), (5, 33, 9, 33, 0.05, "source", 6)]


@pytest.mark.parametrize("case", FRESH, ids=lambda c: "A{}-E{}-H{}-S{}-{}-{}".format(c[0], c[1], c[2], c[3], c[5], c[6]))
@pytest.mark.parametrize("expect,knobs", FORMS)
def test_fresh_trees(ctx, monkeypatch, expect, knobs, case):
    k, episodes, horizon, n_states, rate, rule, max_steps = case
    t, r, term = table(k, 300 + k + episodes, n_states, rate)
    s0 = (np.arange(N) * 5 % n_states).astype(np.int32)
    steps0 = (np.arange(N) % 5).astype(np.int32) if max_steps else np.zeros(N, np.int32)
    rng0 = records(N, 21000 + 100 * k + episodes + horizon)
    p = np.ones(k) / k
    refs = reference(("fresh", case), lambda: oracle_roots(t, r, term, s0, steps0, episodes, horizon, p, rng0, rule, max_steps, horizon))
    if episodes >= 33:
        assert sum(len(partly_visited(ref["tree"], k)) for ref in refs) >= 1, "the case re-enters groups that hold unpicked children"

    def run(expect):
        model = ctx_model(ctx, t, r, term, done_rule=rule, max_steps=max_steps)
        return plan_and_export(ctx, expect, model, s0, episodes, horizon, p, rng0, steps0=steps0 if max_steps else None)
    for arm, (out, rng, trees) in zip(ARMS, run_arms(ctx, monkeypatch, expect, knobs, run)):
        assert_against_oracle(out, rng, trees, refs, arm or "default")


# ---- counts beyond the quotient tables, paths deeper than the registers hold: parents at depth >= 2, whose word is in memory, and
# ---- picks below the levels whose statistics stay in registers, which are stored at their entry ------------------------------------
@pytest.mark.parametrize("expect,knobs", FORMS)
def test_deep_corridor_and_counts_beyond_the_tables(ctx, monkeypatch, expect, knobs):
    k, episodes, horizon = 5, 360, 12
    assert episodes > 16384 // (8 * (k + 1))                  # more counts than the tables hold
    t, r, term = corridor(14, k)
    s0 = (np.arange(N) % 3).astype(np.int32)
    rng0 = records(N, 22000)
    p = np.ones(k) / k
    refs = reference("corridor", lambda: oracle_roots(t, r, term, s0, np.zeros(N, np.int32), episodes, horizon, p, rng0, "source", 0, horizon))
    deepest, deep_partial = 0, 0
    for ref in refs[::8]:
        d = depths(ref["tree"], k)
        deepest = max(deepest, int(d.max()))
        deep_partial += sum(1 for n in partly_visited(ref["tree"], k) if d[n] >= 6)
    assert deepest >= 8, deepest                              # below the levels kept in registers, into the path spill
    assert deep_partial >= 1                                  # a partly visited group whose parent lies below them too

    def run(expect):
        return plan_and_export(ctx, expect, ctx_model(ctx, t, r, term), s0, episodes, horizon, p, rng0)
    for arm, (out, rng, trees) in zip(ARMS, run_arms(ctx, monkeypatch, expect, knobs, run)):
        assert_against_oracle(out, rng, trees, refs, arm or "default")


# ---- reward ties and a low temperature: later entries pick visited children again while unpicked ones remain, and draw among ties --
@pytest.mark.parametrize("expect,knobs", FORMS)
def test_reward_ties_re_pick_among_visited_and_unvisited_children(ctx, monkeypatch, expect, knobs):
    k, episodes, horizon, n_states, temperature = 5, 33, 6, 23, 0.05
    t, _, term = table(k, 91, n_states, 0.0)
    r = (np.random.default_rng(92).integers(0, 2, size=(n_states, k))).astype(np.float64)   # rewards 0.0 and 1.0 only
    s0 = (np.arange(N) * 3 % n_states).astype(np.int32)
    rng0 = records(N, 23000)
    p = np.ones(k) / k
    refs = reference("ties", lambda: oracle_roots(t, r, term, s0, np.zeros(N, np.int32), episodes, horizon, p, rng0, "source", 0, horizon,
                                                  temperature=temperature))
    repicked = 0
    for ref in refs:
        cnt, fc = ref["tree"]["count"], ref["tree"]["first_child"]
        repicked += sum(1 for n in partly_visited(ref["tree"], k) if (cnt[fc[n]:fc[n] + k] >= 2).any())
    assert repicked >= N                                       # a visited child picked again beside children nobody picked

    def run(expect):
        return plan_and_export(ctx, expect, ctx_model(ctx, t, r, term), s0, episodes, horizon, p, rng0, temperature=temperature)
    for arm, (out, rng, trees) in zip(ARMS, run_arms(ctx, monkeypatch, expect, knobs, run)):
        assert_against_oracle(out, rng, trees, refs, arm or "default")


# ---- the descent stops at the horizon on a child nobody stored: the leaf never expands and is stored whole with first_child -1 ------
@pytest.mark.parametrize("expect,knobs", FORMS)
def test_descent_stops_at_the_horizon_on_a_never_stored_child(ctx, monkeypatch, expect, knobs):
    k, episodes, horizon, n_states = 4, 12, 2, 15
    t, r, term = table(k, 93, n_states, 0.0)
    s0 = (np.arange(N) * 2 % n_states).astype(np.int32)
    rng0 = records(N, 24000)
    p = np.ones(k) / k
    refs = reference("horizon", lambda: oracle_roots(t, r, term, s0, np.zeros(N, np.int32), episodes, horizon, p, rng0, "source", 0, horizon))
    for ref in refs[::10]:
        d, cnt, fc = depths(ref["tree"], k), ref["tree"]["count"], ref["tree"]["first_child"]
        assert ((d == horizon) & (cnt >= 1)).any() and ((d == horizon) & (cnt == 0)).any() and (fc[d == horizon] < 0).all()

    def run(expect):
        return plan_and_export(ctx, expect, ctx_model(ctx, t, r, term), s0, episodes, horizon, p, rng0)
    for arm, (out, rng, trees) in zip(ARMS, run_arms(ctx, monkeypatch, expect, knobs, run)):
        assert_against_oracle(out, rng, trees, refs, arm or "default")


# ---- kept trees: re-rooting reads the masked trees by the rule, the next plan continues whole trees with plain words ----------------
def kept_reference(t, r, term, s0, rng0, k, episodes, horizon, p):
    """plan; step (root i continues root i); plan; select (sources repeated, out of order, one unnamed); plan -- on the host"""
    from oracle import oracle
    plan1 = [oracle.uct_plan(t, r, term, int(s0[i]), episodes, horizon, GAMMA, TEMPERATURE, p, p, rng0[i], max_plan_len=horizon)
             for i in range(N)]
    acts1 = (np.arange(N) % k).astype(np.int32)
    kept1 = [oracle.uct_reroot(o["tree"], int(a), k) for o, a in zip(plan1, acts1)]
    states1 = t[s0, acts1].astype(np.int32)
    rng1 = np.stack([o["rng_after"] for o in plan1])
    plan2 = [oracle.uct_plan(t, r, term, int(states1[i]), episodes, horizon, GAMMA, TEMPERATURE, p, p, rng1[i], max_plan_len=horizon,
                             init_tree=kept1[i]) for i in range(N)]
    src = np.array([(7 * j + 3) % N for j in range(N - 6)], np.int32)
    src[5], src[9] = src[4], src[4]                            # one source three times: roots of the old batch go unnamed
    acts2 = ((np.arange(len(src)) * 2 + 1) % k).astype(np.int32)
    kept2 = [oracle.uct_reroot(plan2[q]["tree"], int(a), k) for q, a in zip(src, acts2)]
    states2 = t[states1[src], acts2].astype(np.int32)
    rng2 = records(len(src), 25500)
    plan3 = [oracle.uct_plan(t, r, term, int(states2[j]), episodes, horizon, GAMMA, TEMPERATURE, p, p, rng2[j], max_plan_len=horizon,
                             init_tree=kept2[j]) for j in range(len(src))]
    return dict(plan1=plan1, acts1=acts1, states1=states1, plan2=plan2, src=src, acts2=acts2, states2=states2, rng2=rng2, plan3=plan3)


@pytest.mark.parametrize("expect,knobs", FORMS)
def test_step_tree_and_select_then_plan(ctx, monkeypatch, expect, knobs):
    k, episodes, horizon, n_states = 5, 14, 5, 31
    t, r, term = table(k, 94, n_states, 0.05)
    s0 = (np.arange(N) * 3 % n_states).astype(np.int32)
    rng0 = records(N, 25000)
    p = np.ones(k) / k
    ref = reference("kept", lambda: kept_reference(t, r, term, s0, rng0, k, episodes, horizon, p))
    # among the children stepped into: never expanded (fresh tree next), count 1 (mask 0) and partly visited groups below them
    stepped = [(o["tree"]["count"][1 + a], o["tree"]["first_child"][1 + a]) for o, a in zip(ref["plan1"], ref["acts1"])]
    assert any(c == 1 and fc >= 0 for c, fc in stepped) and any(c >= 3 for c, fc in stepped) and any(fc < 0 for c, fc in stepped)

    def run(expect):
        model = ctx_model(ctx, t, r, term)
        rng = rng0.copy()
        ctx.uct_reset_tree()
        out1 = ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
        assert_form(ctx, expect)
        got1 = (out1, rng.copy(), [ctx.uct_tree(i) for i in range(N)])
        ctx.uct_step_tree(ref["acts1"])
        out2 = ctx.uct_plan(model, ref["states1"], episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
        assert_form(ctx, expect)
        got2 = (out2, rng.copy(), [ctx.uct_tree(i) for i in range(N)])
        ctx.uct_step_tree_select(ref["src"], ref["acts2"])
        rng3 = ref["rng2"].copy()
        out3 = ctx.uct_plan(model, ref["states2"], episodes, horizon, GAMMA, TEMPERATURE, p, p, rng3, max_plan_len=horizon)
        assert_form(ctx, expect)
        got3 = (out3, rng3, [ctx.uct_tree(j) for j in range(len(ref["src"]))])
        ctx.uct_reset_tree()
        return got1, got2, got3
    for arm, (got1, got2, got3) in zip(ARMS, run_arms(ctx, monkeypatch, expect, knobs, run)):
        for got, want, what in ((got1, ref["plan1"], "first plan"), (got2, ref["plan2"], "plan after the step"),
                                (got3, ref["plan3"], "plan after the selection")):
            assert_against_oracle(got[0], got[1], got[2], want, "{} / {}".format(arm or "default", what))


@pytest.mark.parametrize("expect,knobs", FORMS)
def test_trees_right_after_the_re_rooting(ctx, monkeypatch, expect, knobs):
    """Two steps in a row apply the first re-rooting at once: a plan of ZERO further visits cannot be asked for, so the re-rooted
    trees (whole, plain words) are read through the second step's own re-rooting -- the plan after step + step against the
    oracle's, whose kept trees went through uct_reroot twice."""
    from oracle import oracle
    k, episodes, horizon, n_states = 3, 20, 4, 19
    t, r, term = table(k, 95, n_states, 0.0)
    s0 = (np.arange(N) * 3 % n_states).astype(np.int32)
    rng0 = records(N, 25700)
    p = np.ones(k) / k
    a1, a2 = (np.arange(N) % k).astype(np.int32), ((np.arange(N) // 2) % k).astype(np.int32)

    def on_the_host():
        plan1 = [oracle.uct_plan(t, r, term, int(s0[i]), episodes, horizon, GAMMA, TEMPERATURE, p, p, rng0[i], max_plan_len=horizon)
                 for i in range(N)]
        kept = []
        for o, x, y in zip(plan1, a1, a2):
            once = oracle.uct_reroot(o["tree"], int(x), k)
            kept.append(None if once is None else oracle.uct_reroot(once, int(y), k))
        s2 = t[t[s0, a1], a2].astype(np.int32)
        rng1 = np.stack([o["rng_after"] for o in plan1])
        plan2 = [oracle.uct_plan(t, r, term, int(s2[i]), episodes, horizon, GAMMA, TEMPERATURE, p, p, rng1[i], max_plan_len=horizon,
                                 init_tree=kept[i]) for i in range(N)]
        return s2, plan2
    s2, plan2 = reference("twice", on_the_host)

    def run(expect):
        model = ctx_model(ctx, t, r, term)
        rng = rng0.copy()
        ctx.uct_reset_tree()
        ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
        ctx.uct_step_tree(a1)
        ctx.uct_step_tree(a2)
        out = ctx.uct_plan(model, s2, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
        assert_form(ctx, expect)
        got = (out, rng, [ctx.uct_tree(i) for i in range(N)])
        ctx.uct_reset_tree()
        return got
    for arm, got in zip(ARMS, run_arms(ctx, monkeypatch, expect, knobs, run)):
        assert_against_oracle(got[0], got[1], got[2], plan2, arm or "default")


# ---- mp_uct_path_count ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("expect,knobs", FORMS)
def test_path_counts_at_inside_and_below_a_group_with_clear_bits(ctx, monkeypatch, expect, knobs):
    k, episodes, horizon, n_states = 5, 20, 6, 29
    t, r, term = table(k, 96, n_states, 0.0)
    s0 = (np.arange(N) * 3 % n_states).astype(np.int32)
    rng0 = records(N, 26000)
    p = np.ones(k) / k
    refs = reference("paths", lambda: oracle_roots(t, r, term, s0, np.zeros(N, np.int32), episodes, horizon, p, rng0, "source", 0, horizon))

    def paths(tree):
        """action paths ending at a parent whose group holds picked and unpicked children (and at a count-1 parent: none picked),
        at both kinds of child and below an unpicked one, with the oracle tree's answers"""
        par, act, cnt, fc = tree["parent"], tree["action"], tree["count"], tree["first_child"]
        found = []
        for node in partly_visited(tree, k)[:2] + [int(n) for n in np.flatnonzero((cnt == 1) & (fc >= 0))[:1]]:
            path, x = [], node
            while x > 0:
                path.append(int(act[x]))
                x = int(par[x])
            path = path[::-1]
            kids = cnt[fc[node]:fc[node] + k]
            found.append((path, int(cnt[node])))
            for a in range(k):
                found.append((path + [a], int(kids[a])))
            unpicked = int(np.flatnonzero(kids == 0)[0])
            found += [(path + [unpicked, 0], -1), (path + [k], -1)]
        return found
    probes = {i: paths(refs[i]["tree"]) for i in (0, 1, 63, 64, 69)}
    assert all(len(v) >= 2 * (k + 3) for v in probes.values())

    def run(expect):
        model = ctx_model(ctx, t, r, term)
        rng = rng0.copy()
        ctx.uct_reset_tree()
        ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
        assert_form(ctx, expect)
        return {i: [ctx.uct_path_count(i, path) for path, _ in v] for i, v in probes.items()}
    for arm, got in zip(ARMS, run_arms(ctx, monkeypatch, expect, knobs, run)):
        for i, v in probes.items():
            assert got[i] == [want for _, want in v], "{}: root {}".format(arm or "default", i)


# ---- a host-array call split into chunks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("expect,knobs", FORMS)
def test_chunked_host_call_against_the_unsplit_one(ctx, monkeypatch, expect, knobs):
    """chunks are whole multiples of 1024 roots: 1100 roots as 1024 + 76 against one launch, in every arm"""
    k, episodes, horizon, n_states, n = 5, 14, 5, 23, 1100
    t, r, term = table(k, 97, n_states, 0.1)
    s0 = (np.arange(n) * 3 % n_states).astype(np.int32)
    rng0 = records(n, 27000)
    p = np.ones(k) / k
    probe = [0, 63, 64, 1023, 1024, 1087, 1088, 1099]
    got = {}
    for arm in ARMS:
        for chunk in ("", "MP_PIPE_CHUNK=1024"):
            poison(ctx, monkeypatch, knobs)
            set_knobs(monkeypatch, " ".join(x for x in (knobs, arm, chunk) if x))
            model = ctx_model(ctx, t, r, term)
            rng = rng0.copy()
            ctx.uct_reset_tree()
            out = ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon)
            assert_form(ctx, expect)
            got[arm, chunk] = (out, rng, [ctx.uct_tree(i) for i in probe])
    base = got["MP_UCT_TREE_STORES=group", ""]
    for key, (out, rng, trees) in got.items():
        for f in ("plans", "plan_len", "env_steps", "root_child_count", "root_value", "root_child_value"):
            assert np.array_equal(out[f], base[0][f]), (key, f)
        np.testing.assert_array_equal(rng, base[1], err_msg=str(key))
        for i, a, b in zip(probe, trees, base[2]):
            assert_tree(a, b, "{}: root {}".format(key, i))


def teardown_module(module):
    for m in _MODELS:
        m.close()
    del _MODELS[:]
