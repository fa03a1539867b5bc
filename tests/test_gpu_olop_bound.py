"""KL-OLOP's bound on the device, function by function (mp_selftest_olop_bound: the __device__ functions olop_kernel calls,
one input per lane) and the plans whose bounds are NaN.

The function tests hold the device against the reference function's own outputs (tests/golden/kl_bound.npz) on the lattice of
tests/kl_lattice.py.  Their tolerance is derived, not tuned: the host test recomputes ``s``, the largest change of a bound when
every ``log`` result moves by one ulp (no decision of the Newton iteration changes on any point, which it asserts).  The device's
log and numpy's are each within 1 ulp of the true value (asserted here and there), hence up to 2 ulp apart; with every decision
equal the bound follows linearly: 2 s; and doubled once more because the host probe moves every call the same way while real
errors are mixed: 4 s, and never more than the project's 1e-12.

The plan tests reach the NaN code of olop.hip (the finite-difference branch, the first-element rule of olop_first_max, nan_seen
in olop_amax, NaN through backup_to_root and selection_rule) and compare with the reference's outputs (tests/golden/olop_nan.npz)
or the restatement on the same table under the rules of tests/test_gpu_olop.py: discrete fields, NaN and inf positions,
generator records and env steps exactly, finite bounds within 1e-12."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.tree_search.olop import OLOP
from rl_agents_amd.envs import generators
from tests import kl_lattice
from tests import olop_restatement as olr
from tests import test_gpu_each_olop_brue as each
from tests.helpers import assert_form, generator_from
from tests.test_gpu_olop import assert_tree, check_batch, env_of, golden_cases_through_the_agent
from tests.test_olop_bound_host import GOLDEN_BOUND, GOLDEN_NAN, lattice, log_arguments, log_ranges, sensitivity, ulp_error
from tests.test_olop_host import golden_case, names

pytestmark = pytest.mark.gpu

BOUND_TOL = 1e-12
NAN_MAKING = kl_lattice.ULP_BELOW_ONE


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_BOUND)


@pytest.fixture(scope="module")
def znan():
    return np.load(GOLDEN_NAN)


@pytest.fixture(scope="module")
def tolerance():
    return min(4 * sensitivity()["s"], BOUND_TOL)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------ the functions
def test_device_log_is_within_one_ulp_of_a_long_double_log(ctx):
    """The premise of every tolerance below."""
    worst = 0.0
    for x in (log_arguments(), log_ranges()):
        err = ulp_error(ctx.selftest_olop_bound("log", x), x)
        print("device log: {} arguments, max error {:.4f} ulp".format(len(x), err.max()))
        worst = max(worst, float(err.max()))
    assert worst <= 1.0


def test_device_bound_over_the_lattice(ctx, golden, tolerance):
    lat, (ref, ref_its, ref_mask) = lattice(), sensitivity()["base"]
    out, its, mask = ctx.selftest_olop_bound("kl_upper_bound", lat["total"], lat["threshold"], lat["count"])
    want = golden["bound"]
    # the decisions first: a different one moves the bound by up to 1e-2
    assert np.array_equal(its, ref_its), np.flatnonzero(its != ref_its)[:5]
    assert np.array_equal(mask, ref_mask), np.flatnonzero(mask != ref_mask)[:5]
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.isnan(want).sum() > 2000
    assert np.array_equal(np.isinf(out), np.isinf(want)) and np.array_equal(out[np.isinf(want)], want[np.isinf(want)])
    exact = ref_its == 0                          # count == 0 and a == b: no arithmetic beyond one division
    assert (lat["count"][exact] == 0).any() and (lat["count"][exact] > 0).any()
    assert np.array_equal(bits(out[exact]), bits(want[exact]))
    fin = np.isfinite(want)
    dev = np.abs(out[fin] - want[fin])
    print("device bound: {} finite points, max |device - reference| = {:.3e}, {} differ; s = {:.3e}, tolerance {:.3e}".format(
        int(fin.sum()), dev.max(), int((dev > 0).sum()), sensitivity()["s"], tolerance))
    assert dev.max() <= tolerance


def test_a_lane_computes_the_same_bits_whatever_its_neighbours_compute(ctx):
    """One lattice, two orders: dealt so that the lanes of a wave differ in iteration count and NaN points sit between finite
    ones, and sorted by iteration count (the lanes of a wave then leave the loop together)."""
    lat, (ref, ref_its, _) = lattice(), sensitivity()["base"]
    n = len(ref)
    by_its = np.argsort(ref_its, kind="stable")
    stride = -(-n // 64)
    k = np.arange(64 * stride)
    dealt = ((k % 64) * stride + k // 64)
    dealt = by_its[dealt[dealt < n]]                # lane l of a wave takes from the l-th 64th of the sorted list
    assert np.array_equal(np.sort(dealt), np.arange(n))
    waves = ref_its[dealt][:n // 64 * 64].reshape(-1, 64)
    assert np.median([len(np.unique(w)) for w in waves]) >= 4
    nan = np.isnan(ref[dealt])
    assert (nan[1:-1] & ~nan[:-2] & ~nan[2:]).sum() > 100
    results = {}
    for name, order in (("dealt", dealt), ("sorted", by_its)):
        out, its, mask = ctx.selftest_olop_bound("kl_upper_bound", lat["total"][order], lat["threshold"][order], lat["count"][order])
        back = np.empty(n, np.int64)
        back[order] = np.arange(n)
        results[name] = (bits(out)[back], its[back], mask[back])
    nan_bits = np.isnan(ref)                       # (a NaN is a NaN: its payload is not part of the contract)
    for a, b in zip(results["dealt"], results["sorted"]):
        assert np.array_equal(a[~nan_bits], b[~nan_bits])
    assert np.array_equal(np.isnan(results["dealt"][0].view(np.float64)), np.isnan(results["sorted"][0].view(np.float64)))
    assert np.array_equal(results["dealt"][1], results["sorted"][1]) and np.array_equal(results["dealt"][2], results["sorted"][2])


def test_device_divergence_on_the_pairs(ctx, golden, tolerance):
    lat = lattice()
    out = ctx.selftest_olop_bound("bernoulli_kl", lat["p"], lat["q"])
    want = golden["kl"]
    for special in (np.isnan, np.isinf, lambda v: v == 0):
        assert np.array_equal(special(out), special(want)) and special(want).any()
    assert np.array_equal(out[np.isinf(want)], want[np.isinf(want)])
    fin = np.isfinite(want)
    dev = np.abs(out[fin] - want[fin])
    worst = int(np.argmax(dev))
    print("device bernoulli_kl: {} finite pairs, max |device - reference| = {:.3e} at p = {!r}, q = {!r} (value {!r}); tolerance "
          "{:.3e}".format(int(fin.sum()), dev.max(), float(lat["p"][fin][worst]), float(lat["q"][fin][worst]),
                          float(want[fin][worst]), tolerance))
    assert dev.max() <= tolerance


# ------------------------------------------------------------------------------------------------------ NaN bounds in plans
def raw_plan(ctx, tr, rw, term, roots, episodes, horizon, gamma, continuation, thr, rng, available=None, order=None):
    """mp_olop_plan on the table with the env's actions in listing order as the device's columns -> (out, trees in the env's
    labels)."""
    tr, rw = np.asarray(tr), np.asarray(rw, np.float64)
    order = list(range(rw.shape[1])) if order is None else [int(a) for a in order]
    av = None if available is None else np.asarray(available)[:, order]
    model = ctx.load_table(tr[:, order], rw[:, order], term, available=av)
    cont = -1 if continuation == "uniform" else order.index(0)
    out = ctx.olop_plan(model, roots, episodes, horizon, gamma, True, cont, thr, OLOP.value_upper_init(gamma, horizon), rng)
    assert_form(ctx, "olop_global")
    trees = []
    for i in range(len(roots)):
        t = ctx.olop_tree(i, 1 + episodes * horizon * rw.shape[1])
        t["action"] = np.where(t["action"] >= 0, np.asarray(order)[np.maximum(t["action"], 0)], -1).astype(np.int32)
        trees.append(t)
    out["plans"] = np.where(out["plans"] >= 0, np.asarray(order)[np.maximum(out["plans"], 0)], -1)
    model.close()
    return out, trees


def nan_table(states, actions, seed, columns, terminal_rate=0.1):
    tab = generators.random_deterministic(states, actions, seed=seed, terminal_rate=terminal_rate)
    tab["reward"] = np.asarray(tab["reward"], np.float64).copy()
    tab["reward"][:, columns] = NAN_MAKING
    return tab


def test_reference_plans_with_nan_bounds_through_the_agent(znan):
    assert golden_cases_through_the_agent(znan) == len(names(znan)) == 10


def test_reference_plans_with_nan_bounds_through_mp_olop_plan(ctx, znan):
    for name in names(znan):
        case = golden_case(znan, name)
        episodes, horizon = int(case["episodes"]), int(case["horizon"])
        thr = olr.thresholds(str(case["threshold"]), str(case["bound_time"]), episodes)
        rng = case["rng_before"].reshape(1, 6).copy()
        out, trees = raw_plan(ctx, case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"], [int(case["s0"])], episodes,
                              horizon, float(case["gamma"]), str(case["continuation"]), thr, rng, case["available"], case["order"])
        assert out["status"][0] == native.MP_OK, name
        assert out["plans"][0, :out["plan_len"][0]].tolist() == case["plan"].tolist(), name
        assert np.array_equal(rng[0], case["rng_after"]) and int(out["env_steps"][0]) == int(case["env_steps"]), name
        ref = {k: case["tree/" + k] for k in ("parent", "action", "depth", "count", "cum", "mu", "vu", "done")}
        assert np.isnan(ref["mu"]).sum() >= 3, name
        assert_tree(olr.as_bfs(trees[0]), ref, name)
        assert np.isnan(out["root_value"][0]) == np.isnan(ref["vu"][0]), name


@pytest.mark.parametrize("continuation", ["uniform", "zeros"])
@pytest.mark.parametrize("column", [0, 1, 2])
def test_70_roots_with_a_nan_making_column(column, continuation):
    """S = 12, |A| = 3, the NaN-making action listed first, in the middle and last; 70 roots, so a workgroup's tree slots and
    LDS path serve several roots in turn.  M = 9 leaves NaN bounds at the first child under "zeros" (8 visits), M = 30 walks on
    after they have turned finite again."""
    tab = nan_table(12, 3, 20 + column, [column])
    env = env_of(tab["transition"], tab["reward"], tab["terminal"], 0)
    roots = (np.arange(70) * 5 % 12).astype(np.int32)
    for episodes in (9, 30):
        cfg = {"gamma": 0.8, "horizon": 4, "episodes": episodes, "upper_bound": {"type": "kullback-leibler"},
               "continuation_type": continuation}
        out = check_batch(env, cfg, roots, range(70), tree_roots=(0, 1, 35, 69))
        assert np.isnan(out["root_value"]).any()


@pytest.mark.parametrize("where", ["first", "past_64", "both"])
def test_70_actions_with_nan_making_rewards(where):
    """|A| = 70 with 66 or more children per node: the first-element rule, the chunked np.amax and the count-restricted
    selection_rule with the NaN child in the first 64-wide chunk, in the second only, and in both."""
    S, A, late = 10, 70, 41
    order = [int(a) for a in np.random.default_rng(503).permutation(A)]
    for a, at in ((0, 0), (late, 68)):            # action 0 is listed first, action `late` 69th
        order.remove(a)
        order.insert(at, a)
    rs = np.random.default_rng(504)
    avail = np.ones((S, A), bool)
    for s in range(S):                            # three actions missing per state, never the two above: `late` is child 65-68
        avail[s, rs.choice([a for a in range(A) if a not in (0, late)], size=3, replace=False)] = False
    columns = {"first": [0], "past_64": [late], "both": [0, late]}[where]
    tab = nan_table(S, A, 505, columns)
    assert all(64 <= [a for a in order if avail[s, a]].index(late) for s in range(S))
    roots = (np.arange(8) * 3 % S).astype(np.int32)
    for cont in ("uniform", "zeros"):
        env = env_of(tab["transition"], tab["reward"], tab["terminal"], 0, avail, order)
        # (72 episodes: a root's 67 children are first walked in listing order, `late` in the 66th or 67th)
        cfg = {"gamma": 0.9, "horizon": 3, "episodes": 72, "upper_bound": {"type": "kullback-leibler"}, "continuation_type": cont}
        out = check_batch(env, cfg, roots, range(8), available=avail, order=order, tree_roots=(0, 7))
        assert np.isnan(out["root_value"]).any()


def test_a_path_of_70_nodes_with_a_nan_making_column():
    """L = 70: a lane computes the bounds of two path nodes, NaN ones among them."""
    tab = nan_table(25, 3, 506, [1], terminal_rate=0.02)
    env = env_of(tab["transition"], tab["reward"], tab["terminal"], 0)
    cfg = {"gamma": 0.95, "horizon": 70, "episodes": 6, "upper_bound": {"type": "kullback-leibler", "time": "local"},
           "continuation_type": "uniform"}
    out = check_batch(env, cfg, np.arange(25, dtype=np.int32), range(25), tree_roots=(0, 12, 24))
    assert np.isnan(out["root_value"]).any()


def test_thresholds_given_at_the_abi_with_nan_inf_and_zero(ctx):
    """Ordinary rewards; the threshold of an episode is NaN, inf or 0: NaN enters value_upper with one episode's bounds and
    leaves it when a later episode recomputes them."""
    tab = generators.random_deterministic(12, 3, seed=507, terminal_rate=0.1)
    episodes, horizon, gamma = 12, 4, 0.8
    good = 4 * np.log(episodes)
    thr = np.array([good, np.nan, good, 0.0, np.inf, np.nan, good, good, np.inf, 0.0, good, np.nan])
    roots = (np.arange(16) * 7 % 12).astype(np.int32)
    nan_nodes = {}
    for cont in ("uniform", "zeros"):
        for upto in (2, 3, episodes - 1, episodes):      # after the first NaN episode, one later, an ordinary last one, a NaN one
            rng = native.seed_sequence_states([508], 0, len(roots))
            rng0 = rng.copy()
            out, trees = raw_plan(ctx, tab["transition"], tab["reward"], tab["terminal"], roots, upto, horizon, gamma, cont,
                                  thr[:upto], rng)
            nan_nodes[cont, upto] = 0
            for i in range(len(roots)):
                gen = generator_from(rng0[i])
                res = olr.olop_plan(tab["transition"], tab["reward"], tab["terminal"], int(roots[i]), upto, horizon, gamma, True,
                                    thr[:upto], cont, gen)
                assert out["status"][i] == native.MP_OK and res["error"] is None
                assert out["plans"][i, :out["plan_len"][i]].tolist() == res["plan"].tolist(), (cont, upto, i)
                assert np.array_equal(rng[i], native.rng_state_from_generator(gen)), (cont, upto, i)
                assert int(out["env_steps"][i]) == res["env_steps"] == upto * horizon
                assert_tree(trees[i], res, (cont, upto, i))
                assert np.array_equal(trees[i]["state"], res["state"])
                each.assert_bound(out["root_value"][i], res["vu"][0], (cont, upto, i))
                nan_nodes[cont, upto] += int(np.isnan(res["mu"]).sum())
            assert nan_nodes[cont, upto] >= len(roots)
    # NaN bounds left nodes that the episode after the NaN one walked again
    assert nan_nodes["uniform", 3] < nan_nodes["uniform", 2] == 4 * len(roots)


def test_one_mdp_per_root_in_lds_with_nan_making_columns(ctx, monkeypatch):
    """mp_olop_plan_models in the olop_each_lds form: the NaN-making rewards read from the root's table in LDS."""
    monkeypatch.setenv("MP_EACH_MODEL", "lds")
    p = dict(kind="olop", budget=36, gamma=0.8, kl=True, continuation="uniform", episodes=9, horizon=4)
    tabs = [nan_table(12, 3, 60 + k, [k % 3]) for k in range(4)]
    model = each.load(ctx, tabs)
    model_index, local = [3, 0, 3, 1, 2, 0, 1], [0, 5, 11, 7, 2, 9, 4]
    out, _, _ = each.check(ctx, p, tabs, model, model_index, local, range(7), "lds", tree_roots=range(7))
    assert np.isnan(out["root_value"]).any()
    model.close()
