"""Single-model value iteration (mp_vi_solve, mp_vi_solve_v, mp_vi_solve_v_robust, mp_vi_backup, mp_vi_sweeps): every
kernel form by name, every threshold between two forms from both sides, and the stopping logic of every family.

vi_run_impl, vi_dense_launch and vi_dense_exact_launch (csrc/vi.hip) choose among about sixty kernel instantiations; the
call records which one produced the returned values (Context.last_kernel_variant(), one of native.vi_form_names()) and
native.vi_geometry() returns what the launch code computes from a shape, through the functions the launches call.  Here:

  a. FORMS maps every name to the smallest case that selects it; a test without a GPU holds the table to the library's list.
  b. The thresholds -- the single-workgroup kernel's LDS limit, the persistent grid's 64-workgroup cap, whole V in LDS against
     V in pieces -- are taken from vi_geometry, never from a copy of the formulas, and run on both sides.
  c. The stopping ladder: `iterations` of 0, 1, 2, 3, 7, 8 and sw - 3 .. sw + 3 around the sweep sw at which the oracle stops,
     on every family (vi_det_small's three rotating buffers; vi_det_persist's verdict two sweeps late and its separate
     judgement of the last two sweeps, plain and robust; the chained launches, plain and replayed from the captured graph,
     with vi_find_stop and the emit kernel; sparse; dense in numpy's order), as Q and as V; zero rewards (stop at the
     first sweep, Q exactly 0) and gamma = 0 (stop at the second).
  d. The captured graph replayed, re-captured, and replayed after an in-place table update: the same call back to back,
     with Context.vi_graph_captures() held to the captures the sequence allows, so a replay is known to be one.
  e. The matrix-core form (vi_dense_q): its lane-to-column map, 4096-column chunks and 8192-column segments pinned ON BITS
     by one-hot rows whose every other product is an exact zero; ragged tails and tail tiles against the same expression in
     np.longdouble, within the a-priori bound of a dot product summed in any order; row blocks cut differently reassemble
     bit for bit.

The references are the oracle (pinned to the reference's goldens and to numpy) and numpy itself; everything but (e) is
compared on bits: Q, V and sweep counts.
"""
import functools

import numpy as np
import pytest

from tests.helpers import assert_form

GAMMA = 0.5
# every knob of the VI launch code, to be CLEARED before a case sets its own (the give-up and timeout hooks of the persistent
# kernel are only ever cleared here, never set: the tests that own them are elsewhere)
KNOBS = ("MP_VI_NO_SMALL", "MP_VI_NO_PERSIST", "MP_VI_NO_GRAPH", "MP_VI_PERSIST_BLOCK", "MP_VI_PERSIST_GIVE_UP",
         "MP_VI_PERSIST_INJECT_TIMEOUT", "MP_VI_EXACT_V", "MP_VI_EXACT_NO_VLDS", "MP_VI_EXACT_WAVES", "MP_VI_DENSE", "MP_DENSE_NO_SPLIT")
NO_SMALL = {"MP_VI_NO_SMALL": "1"}
CHAIN = {"MP_VI_NO_SMALL": "1", "MP_VI_NO_PERSIST": "1"}
# the (|A|, models) pairs vi_det_persist is instantiated for
PERSIST_PAIRS = [(a, 1) for a in (2, 3, 4, 5, 6, 8)] + [(a, 2) for a in (2, 3, 4, 5, 6, 8)] + [(a, 3) for a in (2, 3, 4, 5)] + \
                [(a, 4) for a in (2, 3, 4)]


@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    c.vi_dense_mode("exact")
    yield c
    c.close()


@pytest.fixture
def knobs(monkeypatch):
    """knobs(env): exactly the knobs in the dict ``env`` are set for the VI launch code, until the next call or the test's end."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def set_(env):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return set_


def a_name(a):
    return str(a) if a in (2, 3, 4, 5, 6, 8) else "any"


# ------------------------------------------------------------------------------------------------------------- problems
class Problem(object):
    """A finite MDP in one of the three modes (robust: M > 1 models), loaded on a context and solved by the oracle."""

    def __init__(self, mode, transition, reward, terminal=None, next_states=None):
        self.mode, self.t, self.r, self.term, self.nxt = mode, transition, reward, terminal, next_states
        self.robust = reward.ndim == 3

    def load(self, ctx):
        if self.mode == "deterministic":
            return ctx.load_table(self.t, self.r, None if self.robust else self.term)
        if self.mode == "sparse":
            return ctx.load_sparse(self.t, self.nxt, self.r, self.term)
        return ctx.load_dense(self.t, self.r, None if self.robust else self.term)

    def oracle_q(self, gamma, iterations):
        from oracle import oracle
        return oracle.vi_solve(self.mode, self.t, self.r, self.term, gamma=gamma, iterations=iterations, next_states=self.nxt,
                               robust=self.robust)

    def oracle_v(self, gamma, iterations):
        from oracle import oracle
        return oracle.vi_solve(self.mode, self.t, self.r, self.term, gamma=gamma, iterations=iterations, next_states=self.nxt,
                               robust=self.robust, state_value=True)

    def with_rewards(self, reward):
        return Problem(self.mode, self.t, reward, self.term, self.nxt)


@functools.lru_cache(maxsize=None)
def det_problem(s, a, m=1, seed=None, reward_scale=1.0):
    """generators.random_deterministic; m > 1: the robust problem of that table and m - 1 generators.rewire copies."""
    from rl_agents_amd.envs import generators
    cfg = generators.random_deterministic(s, a, seed=s + a if seed is None else seed, terminal_rate=0.1)
    if m == 1:
        return Problem("deterministic", cfg["transition"], cfg["reward"] * reward_scale, cfg["terminal"])
    copies = [cfg] + [generators.rewire(cfg, fraction=0.3, seed=i) for i in range(1, m)]
    g = np.random.Generator(np.random.PCG64(1000 + s + a))
    # (every copy its own rewards too: with one reward table the min over models never takes a later model's R)
    rewards = [cfg["reward"]] + [g.random(cfg["reward"].shape) for _ in range(1, m)]
    return Problem("deterministic", np.stack([c["transition"] for c in copies]), np.stack(rewards) * reward_scale)


@functools.lru_cache(maxsize=None)
def dense_problem(s, a, seed=None):
    from rl_agents_amd.envs import generators
    cfg = generators.random_stochastic(s, a, seed=s if seed is None else seed, terminal_rate=0.1)
    return Problem("stochastic", cfg["transition"], cfg["reward"], cfg["terminal"])


@functools.lru_cache(maxsize=None)
def sparse_problem(s, a, b, seed=0):
    from rl_agents_amd.envs import generators
    cfg = generators.random_sparse(s, a, branching=b, seed=seed, terminal_rate=0.1)
    return Problem("sparse", cfg["transition"], cfg["reward"], cfg["terminal"], cfg["next"])


def check_solve(ctx, model, prob, gamma, iterations, form, what="", captures=None):
    """vi_solve and vi_solve_v at `iterations` against the oracle at the same `iterations`, on bits, each on the form meant.
    captures = (c_q, c_v): each of the two is called TWICE back to back; the first call must capture the chain of sweeps
    c_q (c_v) times and the second, whose key is then the cached one, not at all -- it replays."""
    q_ref, sweeps_ref = prob.oracle_q(gamma, iterations)
    v_ref = prob.oracle_v(gamma, iterations)
    for new in (captures[:1], (0,)) if captures else ((None,),):
        before = ctx.vi_graph_captures()
        q, sweeps = ctx.vi_solve(model, gamma, iterations, robust=prob.robust)
        assert_form(ctx, form)
        assert new[0] is None or ctx.vi_graph_captures() - before == new[0], (what, iterations, "Q", new)
        assert sweeps == sweeps_ref, (what, iterations, sweeps, sweeps_ref)
        assert np.array_equal(q, q_ref), (what, iterations, "Q")
    for new in (captures[1:], (0,)) if captures else ((None,),):
        before = ctx.vi_graph_captures()
        v = ctx.vi_solve_v(model, gamma, iterations, robust=prob.robust)
        assert_form(ctx, form)
        assert new[0] is None or ctx.vi_graph_captures() - before == new[0], (what, iterations, "V", new)
        assert np.array_equal(v, v_ref), (what, iterations, "V")
    return q, sweeps


# ------------------------------------------------------------------------------------------ a. every name is reached
def _forms():
    t = {}
    for a in (2, 3, 4, 5, 6, 8, 7):
        t["vi_det_small_a" + a_name(a)] = dict(kind="det", s=70, a=a, m=3 if a in (3, 7) else 1, env={}, iterations=40)
    for a, m in PERSIST_PAIRS:       # S = 600: three workgroups of 256 threads, the last one with 88 states
        t["vi_det_persist_a{}_m{}".format(a, m)] = dict(kind="det", s=600, a=a, m=m, env=NO_SMALL, iterations=40)
    for a in (2, 3, 4, 5, 6, 8, 7):
        m = 2 if a in (4, 7) else 1
        t["vi_det_chain_a" + a_name(a)] = dict(kind="det", s=600, a=a, m=m, env=CHAIN, iterations=7)
        t["vi_det_chain_a" + a_name(a) + "_graph"] = dict(kind="det", s=600, a=a, m=m, env=CHAIN, iterations=40)
    t["vi_sparse"] = dict(kind="sparse", s=60, a=2, b=128, env={}, iterations=40)
    t["vi_sparse_big"] = dict(kind="sparse", s=60, a=2, b=129, env={}, iterations=40)
    for s in (64, 80, 96, 112, 128):  # a row of s <= 128 elements is one leaf of s / 8 eight-element steps
        for place, env in (("lds", {}), ("pieces", {"MP_VI_EXACT_V": "pieces"}), ("global", {"MP_VI_EXACT_V": "global"})):
            t["vi_dense_exact_n{}_{}".format(s // 8, place)] = dict(kind="dense", s=s, a=2, env=env, iterations=40)
    t["vi_dense_mfma"] = dict(kind="mfma", rows=70, a=3, cols=70)
    t["vi_dense_mfma_split"] = dict(kind="mfma", rows=37, a=2, cols=8193)
    return t


FORMS = _forms()


def test_every_vi_form_has_a_case():
    """No GPU: the table above names exactly what the library can record, with no skip list; the dense row lengths select the
    unrolled forms their names say."""
    from rl_agents_amd import native
    names = native.vi_form_names()
    assert len(names) == len(set(names))
    assert set(FORMS) == set(names), set(FORMS) ^ set(names)
    assert not set(names) & set(native.kernel_form_names())
    for name, case in FORMS.items():
        if case["kind"] == "dense":
            g = native.vi_geometry("stochastic", Sc=case["s"])
            assert name == "vi_dense_exact_n{}_{}".format(g["nbt"], name.rsplit("_", 1)[1]), (name, g)
            assert g["v_default"] == "lds" and g["nseg"] == 1
        if case["kind"] == "mfma":
            assert (native.vi_geometry("stochastic", Sc=case["cols"])["nseg"] > 1) == name.endswith("_split")
        if case["kind"] == "det":
            g = native.vi_geometry("deterministic", case["s"], case["a"], case["m"])
            assert g["small_fits"], (name, g)       # (the persistent and chained cases must force their way past it)
            assert g["persist_wgs"] == (1 if case["s"] == 70 else 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FORMS))
def test_form_reached(ctx, knobs, name):
    case = FORMS[name]
    if case["kind"] == "mfma":
        run_mfma_backup(ctx, knobs, case["rows"] * case["a"], case["a"], case["cols"], 2, name)
        return
    if case["kind"] == "det":
        prob = det_problem(case["s"], case["a"], case["m"])
    elif case["kind"] == "sparse":
        prob = sparse_problem(case["s"], case["a"], case["b"])
    else:
        prob = dense_problem(case["s"], case["a"])
    knobs(case["env"])
    model = prob.load(ctx)
    check_solve(ctx, model, prob, GAMMA, case["iterations"], name, name)
    model.close()


@pytest.mark.gpu
@pytest.mark.parametrize("a", [1, 64, 65])
def test_chain_generic_action_counts(ctx, knobs, a):
    """|A| = 1, 64 and 65 take the loop form of the chained sweeps (65 is past what the single-workgroup kernel serves, and
    none has a persistent form), plain and from the graph."""
    prob = det_problem(600, a)
    knobs(CHAIN)
    model = prob.load(ctx)
    check_solve(ctx, model, prob, GAMMA, 7, "vi_det_chain_aany", a)
    check_solve(ctx, model, prob, GAMMA, 40, "vi_det_chain_aany_graph", a)
    model.close()
    if a == 65:     # without any knob too: |A| > 64 never goes to one workgroup, whatever its LDS need
        knobs({})
        small = det_problem(20, a)
        model = small.load(ctx)
        check_solve(ctx, model, small, GAMMA, 40, "vi_det_chain_aany_graph", a)
        model.close()


@pytest.mark.gpu
def test_sweeps_hook_records_its_form(ctx, knobs):
    """mp_vi_sweeps (the timing hook of the benchmark) runs the same launch code and records it."""
    prob = det_problem(600, 5)
    model = prob.load(ctx)
    for env, form in (({}, "vi_det_small_a5"), (NO_SMALL, "vi_det_persist_a5_m1"), (CHAIN, "vi_det_chain_a5_graph")):
        knobs(env)
        ctx.vi_sweeps(model, GAMMA, 12)
        ctx.synchronize()
        assert_form(ctx, form)
    model.close()


# ------------------------------------------------------------------------------------------ b. the thresholds, both sides
def last_true(pred, lo, hi):
    """The largest x in [lo, hi) with pred(x), for a pred that holds up to some x and never after (checked at the ends)."""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def small_limit(a, m, cus=256):
    from rl_agents_amd import native
    return last_true(lambda s: native.vi_geometry("deterministic", s, a, m, cus=cus)["small_fits"], 1, 1 << 16)


def persist_limit(a, m, cus=256):
    from rl_agents_amd import native
    return last_true(lambda s: native.vi_geometry("deterministic", s, a, m, cus=cus)["persist"], 1, 1 << 20)


@functools.lru_cache(maxsize=None)
def v_lds_limit():
    """The last row length whose V sits whole in LDS beside the summation tables.  The tables grow in steps with the row
    length, so the placement need not be monotone in it: every length from one piece (8192) to four is asked, and the
    lengths that take "lds" must be exactly those up to the one returned -- nothing past it fits again."""
    from rl_agents_amd import native
    lds = [sc for sc in range(8192, 4 * 8192 + 1) if native.vi_geometry("stochastic", Sc=sc)["v_default"] == "lds"]
    assert lds == list(range(8192, lds[-1] + 1)), "whole V in LDS is not one run of row lengths"
    return lds[-1]


def test_thresholds_from_geometry(monkeypatch):
    """No GPU: the sizes (b) runs at, as the library reports them; the knobs show in the query as they do in the launch."""
    from rl_agents_amd import native
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for a, m in ((2, 1), (4, 3)):
        s = small_limit(a, m)
        lo, hi = native.vi_geometry("deterministic", s, a, m), native.vi_geometry("deterministic", s + 1, a, m)
        assert lo["small"] and lo["small_fits"] and not hi["small"] and not hi["small_fits"] and hi["persist"]
        assert hi["small_lds"] - lo["small_lds"] == 3 * 8 + m * a * 12     # three V iterates, an int32 and a double per entry
        assert 1 < hi["persist_wgs"] <= 64
    s = persist_limit(2, 1)
    assert s == 16384 and native.vi_geometry("deterministic", s, 2, 1)["persist_wgs"] == 64
    assert native.vi_geometry("deterministic", s + 1, 2, 1)["persist_wgs"] == 65
    assert not native.vi_geometry("deterministic", 600, 7, 1)["persist"]        # no instantiation
    assert not native.vi_geometry("deterministic", 600, 5, 4)["persist"]
    assert not native.vi_geometry("deterministic", 600, 5, 1, cus=2)["persist"]  # three workgroups on two compute units
    sc = v_lds_limit()
    lo, hi = native.vi_geometry("stochastic", Sc=sc), native.vi_geometry("stochastic", Sc=sc + 1)
    assert (lo["v_default"], hi["v_default"]) == ("lds", "pieces") and lo["v"] == "lds" and hi["v"] == "pieces"
    assert lo["nseg"] == -(-sc // 8192) and lo["seg_cols"] == 8192
    monkeypatch.setenv("MP_VI_NO_SMALL", "1")
    g = native.vi_geometry("deterministic", 70, 2, 1)
    assert g["small_fits"] and not g["small"] and g["persist"]
    monkeypatch.setenv("MP_VI_NO_PERSIST", "1")
    assert not native.vi_geometry("deterministic", 70, 2, 1)["persist"]
    monkeypatch.setenv("MP_VI_EXACT_V", "global")
    g = native.vi_geometry("stochastic", Sc=96)
    assert (g["v_default"], g["v"]) == ("lds", "global")
    monkeypatch.setenv("MP_VI_EXACT_V", "pieces")
    assert native.vi_geometry("stochastic", Sc=96)["v"] == "pieces"
    monkeypatch.setenv("MP_VI_EXACT_NO_VLDS", "1")
    assert native.vi_geometry("stochastic", Sc=96)["v"] == "global"
    monkeypatch.setenv("MP_DENSE_NO_SPLIT", "1")
    assert native.vi_geometry("stochastic", Sc=sc)["nseg"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("a,m", [(2, 1), (4, 3)])
def test_single_workgroup_limit(ctx, knobs, a, m):
    """The last S whose tables fit one workgroup's LDS runs there; S + 1 on the persistent grid."""
    cus = ctx.device_info()["n_cu"]
    s = small_limit(a, m, cus)
    for n, form in ((s, "vi_det_small_a{}".format(a)), (s + 1, "vi_det_persist_a{}_m{}".format(a, m))):
        prob = det_problem(n, a, m)
        model = prob.load(ctx)
        check_solve(ctx, model, prob, GAMMA, 40, form, n)
        model.close()


@pytest.mark.gpu
def test_persistent_grid_cap(ctx, knobs):
    """64 workgroups are the most the persistent kernel is given; one state more goes to the chained sweeps."""
    cus = ctx.device_info()["n_cu"]
    s = persist_limit(2, 1, cus)
    assert s == 16384
    for n, form in ((s, "vi_det_persist_a2_m1"), (s + 1, "vi_det_chain_a2_graph")):
        prob = det_problem(n, 2)
        model = prob.load(ctx)
        check_solve(ctx, model, prob, GAMMA, 40, form, n)
        model.close()


@pytest.mark.gpu
def test_whole_v_in_lds_limit(ctx, knobs):
    """The last row length with all of V in LDS, and the next one, which stages it in pieces: a 37-row block, two models,
    against numpy's own expression and the oracle."""
    from oracle import oracle
    from rl_agents_amd import native
    sc = v_lds_limit()
    for n, place in ((sc, "lds"), (sc + 1, "pieces")):
        g = np.random.Generator(np.random.PCG64(n))
        t = g.random((2, 37, 2, n))
        t /= t.sum(-1, keepdims=True)
        r = g.random((2, 37, 2))
        v = g.standard_normal(n) * 3
        blk = ctx.load_dense_rows(t, r, None)
        q = ctx.vi_backup(blk, 0.95, v, robust=True)
        assert_form(ctx, "vi_dense_exact_n{}_{}".format(native.vi_geometry("stochastic", Sc=n)["nbt"], place))
        ref = np.min(r + 0.95 * (t * v.reshape((1, 1, 1, v.size))).sum(axis=-1), axis=0)   # robust_value_iteration.py:46-58
        assert np.array_equal(q, ref), n
        assert np.array_equal(q, oracle.dense_backup_rows(t, r, None, v, 0.95, robust=True)), n
        blk.close()


# ------------------------------------------------------------------------------------------ c. the stopping ladder
# family -> (problems, knobs, form at `iterations`)
def _chain_form(a, graph):
    # (0 sweeps of the chained launches, as of a sparse or dense model, launch no sweep: the empty name)
    return lambda iterations: "vi_det_chain_a{}{}".format(a_name(a), "_graph" if graph and iterations >= 8 else "") if iterations else ""


def _ladder_problems(m):
    # sw = 19; and rewards x 1e-6 (the absolute tolerance ends it): sw = 8, exactly where the graph takes over
    return [("det257", det_problem(257, 3, m, seed=260), 3), ("det300", det_problem(300, 4, m, seed=0, reward_scale=1e-6), 4)]


def _families():
    f = {}
    f["small"] = ([(n, p, lambda it, a=a: "vi_det_small_a{}".format(a)) for n, p, a in _ladder_problems(1)], {})
    f["persist"] = ([(n, p, lambda it, a=a: "vi_det_persist_a{}_m1".format(a)) for n, p, a in _ladder_problems(1)], NO_SMALL)
    f["persist_robust"] = ([(n, p, lambda it, a=a: "vi_det_persist_a{}_m2".format(a)) for n, p, a in _ladder_problems(2)], NO_SMALL)
    f["chain_plain"] = ([(n, p, _chain_form(a, False)) for n, p, a in _ladder_problems(1)], dict(CHAIN, MP_VI_NO_GRAPH="1"))
    f["chain_graph"] = ([(n, p, _chain_form(a, True)) for n, p, a in _ladder_problems(1)], CHAIN)
    f["chain_graph_robust"] = ([(n, p, _chain_form(a, True)) for n, p, a in _ladder_problems(2)], CHAIN)
    f["sparse"] = ([("sparse100", sparse_problem(100, 3, 4), lambda it: "vi_sparse" if it else "")], {})
    f["dense_exact"] = ([("dense96", dense_problem(96, 2), lambda it: "vi_dense_exact_n12_lds" if it else "")], {})
    return f


FAMILIES = ("small", "persist", "persist_robust", "chain_plain", "chain_graph", "chain_graph_robust", "sparse", "dense_exact")
LADDER_SW = {"det257": 19, "det300": 8, "sparse100": 17, "dense96": 16}


def ladder(sw):
    return sorted(set([0, 1, 2, 3, 7, 8] + [sw + d for d in range(-3, 4)]))


def zero_rewards(prob):
    return prob.with_rewards(np.zeros_like(prob.r))


def test_ladder_problems_stop_where_the_ladder_stands():
    """No GPU: the oracle's stopping sweep of every ladder problem (200 iterations allowed) is inside [8, 40] and is the one
    the comments name, so that the ladder really has rungs on both sides of the verdict, of the post-loop judgement of the
    last two sweeps, and of the graph threshold; zero rewards stop at the first sweep, gamma = 0 at the second."""
    fams = _families()
    assert set(fams) == set(FAMILIES)
    for fam in FAMILIES:
        for name, prob, _ in fams[fam][0]:
            sw = prob.oracle_q(GAMMA, 200)[1]
            assert 8 <= sw <= 40, (fam, name, sw)
            assert sw == LADDER_SW[name], (fam, name, sw)
            q, s1 = zero_rewards(prob).oracle_q(GAMMA, 40)
            assert s1 == 1 and not q.any()
            assert prob.oracle_q(0.0, 40)[1] == 2
    assert LADDER_SW["det300"] == 8      # the first `iterations` replayed from the graph
    assert ladder(19) == [0, 1, 2, 3, 7, 8, 16, 17, 18, 19, 20, 21, 22]


def graph_captures(family, iterations):
    """What check_solve is to hold the capture count to: on the graph families every rung from 8 sweeps up is a new key as Q
    and again as V (one capture each), then replayed; below 8 sweeps, and on every other family, nothing is ever captured."""
    if family.startswith("chain_graph"):
        return (1, 1) if iterations >= 8 else (0, 0)
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_stopping_ladder(ctx, knobs, family):
    """Every rung on bits against the oracle.  On the graph families each call comes twice: captured, then replayed."""
    problems, env = _families()[family]
    knobs(env)
    for name, prob, form in problems:
        sw = prob.oracle_q(GAMMA, 200)[1]
        assert 8 <= sw <= 40
        model = prob.load(ctx)
        for iterations in ladder(sw):
            _, sweeps = check_solve(ctx, model, prob, GAMMA, iterations, form(iterations), (family, name),
                                    graph_captures(family, iterations))
            assert sweeps == min(iterations, sw)
        model.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_stops_at_the_first_and_second_sweep(ctx, knobs, family):
    """Zero rewards: Q_1 = Q_0 = 0, the first sweep's test passes (j = 0: the iterate returned is the initial one).
    gamma = 0: Q_1 = R = Q_2, the second sweep's does (j = 1).  Both below the persistent kernel's lag."""
    problems, env = _families()[family]
    knobs(env)
    name, prob, form = problems[0]
    zero = zero_rewards(prob)
    model = zero.load(ctx)
    for iterations in (1, 2, 3, 9, 40):
        q, sweeps = check_solve(ctx, model, zero, GAMMA, iterations, form(iterations), (family, "zero"),
                                graph_captures(family, iterations))
        assert sweeps == 1 and not q.any()
    model.close()
    model = prob.load(ctx)
    for iterations in (1, 2, 3, 4, 9, 40):
        q, sweeps = check_solve(ctx, model, prob, 0.0, iterations, form(iterations), (family, "gamma0"),
                                graph_captures(family, iterations))
        assert sweeps == min(iterations, 2)
        if iterations >= 2:
            assert np.array_equal(q, np.min(prob.r, axis=0) if prob.robust else prob.r)
    model.close()


# ------------------------------------------------------------------------------------------ d. the captured graph
@pytest.mark.gpu
def test_graph_replayed_recaptured_and_replayed_on_new_tables(ctx, knobs):
    """One context, one model, 40 sweeps.  The context keeps the executable graph of its last chain, keyed by everything its
    kernel arguments hold; a call with that key replays it, any other captures anew.  `_graph` is recorded either way, so
    every step holds Context.vi_graph_captures() to what the step may capture: identical calls come back to back with no
    other VI call between them, and the second one must find its key and leave the count alone.  After an in-place table
    update the call that ran last comes again -- same pointers, same key, no capture -- and the replayed graph must solve
    the NEW tables.  Every step on bits against the oracle."""
    from rl_agents_amd.envs import generators
    knobs(CHAIN)
    form = "vi_det_chain_a3_graph"
    prob = det_problem(257, 3, seed=260)
    cfg = generators.rewire(dict(transition=prob.t), fraction=0.5, seed=9)
    new = Problem("deterministic", cfg["transition"], np.random.Generator(np.random.PCG64(9)).random(prob.r.shape), prob.term)
    assert not np.array_equal(new.oracle_q(GAMMA, 40)[0], prob.oracle_q(GAMMA, 40)[0])
    assert not np.array_equal(new.oracle_v(GAMMA, 40), prob.oracle_v(GAMMA, 40))
    model = prob.load(ctx)

    def solve_q(p, gamma, captures, what):
        before = ctx.vi_graph_captures()
        q, sweeps = ctx.vi_solve(model, gamma, 40)
        assert_form(ctx, form)
        assert ctx.vi_graph_captures() - before == captures, what
        q_ref, sweeps_ref = p.oracle_q(gamma, 40)
        assert sweeps == sweeps_ref and np.array_equal(q, q_ref), what

    def solve_v(p, gamma, captures, what):
        before = ctx.vi_graph_captures()
        v = ctx.vi_solve_v(model, gamma, 40)
        assert_form(ctx, form)
        assert ctx.vi_graph_captures() - before == captures, what
        assert np.array_equal(v, p.oracle_v(gamma, 40)), what

    solve_q(prob, 0.8, 1, "gamma = 0.8 first (no other case of this module solves at it, so the key is new)")
    solve_q(prob, GAMMA, 1, "capture")
    solve_q(prob, GAMMA, 0, "replay")
    solve_q(prob, GAMMA, 0, "replay again")
    solve_q(prob, 0.8, 1, "another gamma re-captures")
    solve_q(prob, 0.8, 0, "and replays")
    solve_q(prob, GAMMA, 1, "back: one graph is kept, not one per key")
    solve_q(prob, GAMMA, 0, "replay")
    model.update_tables(0, new.t, new.r, new.term)
    solve_q(new, GAMMA, 0, "the call that ran last, replayed on the new tables")
    solve_q(new, GAMMA, 0, "and again")
    solve_v(new, GAMMA, 1, "the V form is another key")
    solve_v(new, GAMMA, 0, "replay")
    model.update_tables(0, prob.t, prob.r, prob.term)
    solve_v(prob, GAMMA, 0, "the V form replayed on the first tables put back")
    solve_q(prob, GAMMA, 1, "the Q form again")
    model.close()


# ------------------------------------------------------------------------------------------ e. the matrix cores
U = 2.0 ** -53
MFMA_COLS = (1, 5, 15, 16, 17, 4095, 4096, 4097, 8192, 8193, 16385)
MFMA_ROWS = ((1, 1), (15, 3), (63, 3), (64, 2), (65, 5))     # (S * A, A): no tile, ragged tiles, one tile, one row into the next


@functools.lru_cache(maxsize=4)
def mfma_data(sa, a, cols):
    """Two models of sa / a source rows: T normalised with 30 % exact zeros, R and V = 3 N(0, 1), a terminal mask."""
    g = np.random.Generator(np.random.PCG64(cols * 100 + sa))
    rows = sa // a
    t = g.random((2, rows, a, cols))
    t[g.random(t.shape) < 0.3] = 0.0
    t /= np.maximum(t.sum(-1, keepdims=True), 1e-300)
    r = g.standard_normal((2, rows, a))
    v = g.standard_normal(cols) * 3
    term = g.random(rows) < 0.3
    if rows > 1:
        term[0], term[-1] = True, False
    return t, r, v, term


def mfma_reference(t, r, v, term, gamma):
    """The backup in np.longdouble and the a-priori error bound of a double-precision evaluation in ANY order, per output:
    a dot product of n rounded or fused products summed in any order errs by at most gamma_n sum |T_j V_j| (Higham, Accuracy
    and Stability of Numerical Algorithms, 3.1), and R + gamma x adds two roundings: gamma_(n + 2) (|R| + gamma sum |T_j V_j|),
    gamma_n = n u / (1 - n u).  t [M, rows, A, cols]; term None for the robust min, whose bound is the models' largest."""
    ld = np.longdouble
    n = t.shape[-1] + 2
    gam_n = ld(n) * ld(U) / (1 - ld(n) * ld(U))
    prod = t.astype(ld) * v.astype(ld)
    nv, mag = prod.sum(-1), np.abs(prod).sum(-1)
    if term is not None:
        nv[:, term] = 0
        mag[:, term] = 0
    q = r.astype(ld) + ld(gamma) * nv
    bound = gam_n * (np.abs(r).astype(ld) + ld(gamma) * mag)
    return q.min(axis=0), bound.max(axis=0)


def test_oracle_meets_the_matrix_core_bound():
    """No GPU: numpy's own order (the oracle) lies inside the bound the matrix-core form is held to, on every shape of (e) --
    a wrong reference or a wrong bound fails here."""
    from oracle import oracle
    for cols in MFMA_COLS:
        for sa, a in MFMA_ROWS:
            t, r, v, term = mfma_data(sa, a, cols)
            ref, bound = mfma_reference(t[:1], r[:1], v, term, 0.95)
            got = oracle.dense_backup_rows(t[0], r[0], term, v, 0.95)
            assert np.all(np.abs(got.astype(np.longdouble) - ref) <= bound), (cols, sa)
            ref, bound = mfma_reference(t, r, v, None, 0.95)
            got = oracle.dense_backup_rows(t, r, None, v, 0.95, robust=True)
            assert np.all(np.abs(got.astype(np.longdouble) - ref) <= bound), (cols, sa)
            assert np.all(bound < 1e-11)


def run_mfma_backup(ctx, knobs, sa, a, cols, models, form=None):
    """One backup of a row block on the matrix cores: plain with a terminal mask (models = 1) or the robust min, inside the
    bound; the form recorded is the split one exactly when vi_geometry says the columns are cut."""
    from rl_agents_amd import native
    knobs({})
    want = "vi_dense_mfma_split" if native.vi_geometry("stochastic", Sc=cols)["nseg"] > 1 else "vi_dense_mfma"
    assert form in (None, want)
    t, r, v, term = mfma_data(sa, a, cols)
    ctx.vi_dense_mode("mfma")
    try:
        for m in range(1, models + 1):
            robust = m > 1
            blk = ctx.load_dense_rows(t if robust else t[0], r if robust else r[0], None if robust else term)
            q = ctx.vi_backup(blk, 0.95, v, robust=robust)
            assert_form(ctx, want)
            blk.close()
            ref, bound = mfma_reference(t[:m], r[:m], v, None if robust else term, 0.95)
            err = np.abs(q.astype(np.longdouble) - ref)
            assert np.all(err <= bound), (cols, sa, m, float((err / bound).max()))
            if not robust and term.any():
                assert np.array_equal(q[term], r[0][term])       # (masked rows: R + gamma * 0)
    finally:
        ctx.vi_dense_mode("exact")


@pytest.mark.gpu
@pytest.mark.parametrize("cols", MFMA_COLS)
def test_matrix_cores_shape_edges(ctx, knobs, cols):
    """Ragged tails of a row (cols % 16), chunk and segment boundaries, a one-column last segment; tail tiles (S A % 64)."""
    for sa, a in MFMA_ROWS:
        run_mfma_backup(ctx, knobs, sa, a, cols, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [8192, 8193, 16385])
def test_matrix_cores_column_map_on_bits(ctx, knobs, cols):
    """40 rows, |A| = 1, each one-hot at a column c with V[c] = c + 1: every other product is an exact zero, so whatever the
    order of the additions Q = R + gamma (c + 1) ON BITS.  A lane that multiplies a column of T with another column's V, a
    chunk or a segment that starts one column off, or a column dropped at an end returns R + gamma * 0 or another c."""
    knobs({})
    edge = [c for c in (0, 3, 4, 15, 16, 4095, 4096, 8191, 8192, cols - 1) if c < cols]
    g = np.random.Generator(np.random.PCG64(cols))
    # (the other rows: every lane slot of a 16-column step, and columns anywhere)
    cs = np.array(edge + list(range(32, 48)) + list(g.integers(0, cols, size=40 - 16 - len(edge))))
    assert len(cs) == 40
    t = np.zeros((40, 1, cols))
    t[np.arange(40), 0, cs] = 1.0
    r = g.standard_normal((40, 1))
    v = np.arange(cols, dtype=np.float64) + 1.0
    ctx.vi_dense_mode("mfma")
    try:
        blk = ctx.load_dense_rows(t, r, None)
        q = ctx.vi_backup(blk, 0.95, v)
        assert_form(ctx, "vi_dense_mfma_split" if cols > 8192 else "vi_dense_mfma")
        blk.close()
    finally:
        ctx.vi_dense_mode("exact")
    want = r + 0.95 * (cs + 1.0).reshape(40, 1)
    bad = np.flatnonzero(q[:, 0] != want[:, 0])
    assert bad.size == 0, "rows one-hot at columns {} came back as V[{}]".format(cs[bad], (q[bad, 0] - r[bad, 0]) / 0.95 - 1)


@pytest.mark.gpu
def test_matrix_cores_row_blocks_reassemble(ctx, knobs):
    """With the columns split, a row's result depends on its columns only: 40 rows as one block and as 17 + 23 (the tail
    tiles fall differently) are bit-equal.  (Nothing claims equality with the unsplit sum, and none is asserted.)"""
    knobs({})
    t, r, v, term = mfma_data(80, 2, 8193)
    ctx.vi_dense_mode("mfma")
    try:
        for robust in (False, True):
            parts = []
            for lo, hi in ((0, 40), (0, 17), (17, 40)):
                tt, rr = (t[:, lo:hi], r[:, lo:hi]) if robust else (t[0, lo:hi], r[0, lo:hi])
                blk = ctx.load_dense_rows(tt, rr, None if robust else term[lo:hi])
                parts.append(ctx.vi_backup(blk, 0.95, v, robust=robust))
                assert_form(ctx, "vi_dense_mfma_split")
                blk.close()
            assert np.array_equal(parts[0], np.concatenate(parts[1:])), robust
    finally:
        ctx.vi_dense_mode("exact")
