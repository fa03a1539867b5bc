"""OLOP and BRUE on a batch model with one MDP per root (mp_olop_plan_models / mp_brue_plan_models, the `_each_lds` and
`_each_global` kernel forms) against the test-side restatements (tests/olop_restatement.py, tests/brue_restatement.py) run on
each root's OWN table alone.

Parity: status, plans, env steps, generator records, BRUE's root value and every discrete field of the trees on bits; OLOP's
bounds (mu_ucb / value_upper) within 1e-12, the project's tolerance for the device's log in the KL bound's Newton step
(DESIGN.md 4.6).  Exported trees hold GLOBAL states, model_index * S_each + local."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.tree_search.brue import BRUE
from rl_agents_amd.agents.tree_search.olop import OLOP
from rl_agents_amd.envs import generators
from tests import brue_restatement as brr
from tests import olop_restatement as olr
from tests.helpers import assert_form, generator_from

pytestmark = pytest.mark.gpu

BOUND_TOL = 1e-12
KEEP_BYTES = 1 << 30            # trees of every root are kept while they fit (kOlopKeepBytes / kBrueKeepBytes)
KL_UNIFORM = dict(kind="olop", budget=100, gamma=0.8, kl=True, continuation="uniform")
HOEFFDING_ZEROS = dict(kind="olop", budget=100, gamma=0.8, kl=False, continuation="zeros")
BRUE_60 = dict(kind="brue", budget=60, gamma=0.8)
PLANS = [pytest.param(KL_UNIFORM, id="olop-kl-uniform"), pytest.param(HOEFFDING_ZEROS, id="olop-hoeffding-zeros"),
         pytest.param(BRUE_60, id="brue")]
FORMS = ["lds", "global"]


@pytest.fixture(scope="module")
def ctx():
    return native.Context(0)


def sized(plan):
    """The plan's config with what the agents' host code derives from it: OLOP's episodes / horizon (olop.py:50-62), BRUE's
    horizon (the same split) unless they are given."""
    p = dict(plan)
    if "horizon" not in p:
        p["episodes"], p["horizon"] = native.olop_allocation(p["budget"], p["gamma"])
    return p


def stack(tabs):
    return (np.stack([t["transition"] for t in tabs]).astype(np.int64), np.stack([t["reward"] for t in tabs]).astype(np.float64),
            np.stack([np.asarray(t["terminal"]) for t in tabs]).astype(np.uint8))


def load(ctx, tabs, available=None, order=None):
    """The batch model of `tabs`; with a listing order the device's columns are the env's actions in that order."""
    t, r, term = stack(tabs)
    if order is not None:
        t, r = t[:, :, order], r[:, :, order]
    model = ctx.load_table_batch(t, r, term)
    if available is not None:
        av = np.stack(available)
        model.set_available(av[:, :, order].reshape(-1, av.shape[2]) if order is not None else av.reshape(-1, av.shape[2]))
    return model


def device_plan(ctx, model, p, model_index, local, rng, order=None):
    mi, ls = np.asarray(model_index, np.int32), np.asarray(local, np.int32)
    if p["kind"] == "brue":
        return ctx.brue_plan(model, ls, p["budget"], p["horizon"], p["gamma"], BRUE.gamma_powers(p["gamma"], p["horizon"]), rng,
                             model_index=mi)
    thr = olr.thresholds("4*np.log(time)", "global", p["episodes"]) if p["kl"] else np.zeros(0)
    cont = -1 if p["continuation"] == "uniform" else (0 if order is None else list(order).index(0))
    return ctx.olop_plan(model, ls, p["episodes"], p["horizon"], p["gamma"], p["kl"], cont, thr,
                         OLOP.value_upper_init(p["gamma"], p["horizon"]), rng, model_index=mi)


def restated(p, tab, s0, rng6, available=None, order=None):
    """The restatement on ONE table from LOCAL state s0 -> (result, generator record after)."""
    gen = generator_from(rng6)
    if p["kind"] == "brue":
        res = brr.brue_plan("deterministic", tab["transition"], tab["reward"], tab["terminal"], int(s0), p["budget"], p["horizon"],
                            p["gamma"], gen)
    else:
        thr = olr.thresholds("4*np.log(time)", "global", p["episodes"]) if p["kl"] else None
        res = olr.olop_plan(tab["transition"], tab["reward"], tab["terminal"], int(s0), p["episodes"], p["horizon"], p["gamma"],
                            p["kl"], thr, p["continuation"], gen, available=available, order=order)
    return res, native.rng_state_from_generator(gen)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def assert_bound(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin, inf = np.isfinite(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what        # (a NaN by position: its sign and payload are no one's contract)
    assert np.array_equal(bits(got[inf]), bits(want[inf])), what
    assert np.all(np.abs(got[fin] - want[fin]) <= BOUND_TOL), (what, np.abs(got[fin] - want[fin]).max())


def assert_root(p, out, rng, i, res, rng_after, order=None):
    assert res.get("error") is None and int(out["status"][i]) == native.MP_OK, i
    assert np.array_equal(rng[i], rng_after), i
    assert int(out["env_steps"][i]) == res["env_steps"], i
    if p["kind"] == "brue":
        assert [int(out["plans"][i])] == res["plan"].tolist(), i
        assert bits(out["root_value"][i]) == bits(res["root_value"]), i
    else:
        n = int(out["plan_len"][i])
        got = out["plans"][i, :n] if order is None else np.asarray(order)[out["plans"][i, :n]]
        assert got.tolist() == res["plan"].tolist(), i
        assert_bound(out["root_value"][i], res["vu"][0], i)


def assert_tree(ctx, p, n_actions, i, res, base, order=None):
    """Root i's whole exported tree == the restatement's, its states moved to the MDP's block of GLOBAL states."""
    if p["kind"] == "brue":
        tree = ctx.brue_tree(i, 1 + 2 * (p["budget"] + p["horizon"]))
        key = np.where((np.asarray(res["is_chance"]) == 0) & (np.asarray(res["parent"]) >= 0), np.asarray(res["key"]) + base, res["key"])
        for k in ("parent", "is_chance", "depth", "count"):
            assert np.array_equal(tree[k], res[k]), (i, k)
        assert np.array_equal(tree["key"], key), (i, "key")
        assert np.array_equal(bits(tree["stat"]), bits(res["stat"])), (i, "stat")
        return
    tree = ctx.olop_tree(i, 1 + p["episodes"] * p["horizon"] * n_actions)
    action = tree["action"] if order is None else np.where(tree["action"] >= 0, np.asarray(order)[np.maximum(tree["action"], 0)], -1)
    assert np.array_equal(action, res["action"]), (i, "action")
    for k in ("parent", "depth", "count", "done"):
        assert np.array_equal(tree[k], res[k]), (i, k)
    assert np.array_equal(bits(tree["cum"]), bits(res["cum"])), (i, "cum")
    assert np.array_equal(tree["state"], np.asarray(res["state"]) + base), (i, "state")
    assert_bound(tree["mu"], res["mu"], (i, "mu"))
    assert_bound(tree["vu"], res["vu"], (i, "vu"))


def keeps_trees(p, n_actions, n_roots):
    """The host's arithmetic for `_slots`: a tree per root while the batch's trees fit the kept workspace."""
    if p["kind"] == "brue":
        per_tree = (1 + 2 * (p["budget"] + p["horizon"])) * (32 + 4 * n_actions)
    else:
        per_tree = (1 + p["episodes"] * p["horizon"] * n_actions) * (48 + 8)
    return n_roots * per_tree <= KEEP_BYTES


def form_name(p, form, keep=True):
    return "{}_each_{}{}".format(p["kind"], form, "" if keep else "_slots")


def check(ctx, p, tabs, model, model_index, local, sample, form, tree_roots=(), available=None, order=None):
    n, s_each, n_actions = len(model_index), tabs[0]["reward"].shape[0], tabs[0]["reward"].shape[1]
    rng = native.seed_sequence_states([11], 0, n)
    rng0 = rng.copy()
    out = device_plan(ctx, model, p, model_index, local, rng, order)
    keep = keeps_trees(p, n_actions, n)
    assert_form(ctx, form_name(p, form, keep))
    for i in sample:
        m = int(model_index[i])
        res, rng_after = restated(p, tabs[m], local[i], rng0[i], None if available is None else available[m], order)
        assert_root(p, out, rng, i, res, rng_after, order)
        if i in tree_roots:
            assert keep or i == 0
            assert_tree(ctx, p, n_actions, i, res, m * s_each, order)
    return out, rng0, rng


# ------------------------------------------------------------------------------------------------------------ 1. own tables
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("plan", PLANS)
def test_every_root_plans_on_its_own_table(ctx, monkeypatch, plan, form):
    monkeypatch.setenv("MP_EACH_MODEL", form)
    p = sized(plan)
    tabs = [generators.random_deterministic(12, 3, seed=k, terminal_rate=0.2) for k in range(4)]
    model = load(ctx, tabs)
    model_index, local = [3, 0, 3, 1, 2, 0, 1], [0, 5, 11, 7, 2, 9, 4]
    out, rng0, _ = check(ctx, p, tabs, model, model_index, local, range(7), form, tree_roots=(0, 2))
    # ... and equal to the plain entry point on the batch model's global states, where it takes them (BRUE's refuses batch models)
    if p["kind"] == "olop":
        rng = rng0.copy()
        thr = olr.thresholds("4*np.log(time)", "global", p["episodes"]) if p["kl"] else np.zeros(0)
        ref = ctx.olop_plan(model, np.asarray(model_index) * 12 + np.asarray(local), p["episodes"], p["horizon"], p["gamma"], p["kl"],
                            -1 if p["continuation"] == "uniform" else 0, thr, OLOP.value_upper_init(p["gamma"], p["horizon"]), rng)
        assert_form(ctx, "olop_global")
        for k in ("plans", "plan_len", "env_steps", "status"):
            assert np.array_equal(out[k], ref[k]), k
        assert np.array_equal(bits(out["root_value"]), bits(ref["root_value"]))
    else:
        with pytest.raises(native.NativeError) as e:
            ctx.brue_plan(model, np.asarray(local), p["budget"], p["horizon"], p["gamma"], BRUE.gamma_powers(p["gamma"], p["horizon"]),
                          rng0.copy())
        assert e.value.code == native.MP_ERR_MODE
    model.close()


# ------------------------------------------------------------------------------------- 2. more roots than workgroups (stale LDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("plan", [pytest.param(dict(kind="olop", budget=8, gamma=0.8, kl=True, continuation="uniform", episodes=4,
                                                    horizon=2), id="olop"),
                                  pytest.param(dict(kind="brue", budget=6, gamma=0.8, horizon=2), id="brue")])
def test_a_workgroup_reloads_the_table_of_its_next_root(ctx, monkeypatch, plan, form):
    """Every workgroup plans at least two roots, and consecutive roots of one workgroup own different tables: a root served
    from the previous root's LDS copy would plan on the wrong MDP."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    p = sized(plan)
    cus = ctx.device_info()["n_cu"]
    grid = native.each_form_info(p["kind"], 6, 2, p["horizon"], 1 << 30, cus)["grid"]
    n = 2 * grid + 3
    info = native.each_form_info(p["kind"], 6, 2, p["horizon"], n, cus)
    assert info["grid"] == grid and info["lds"] == (form == "lds")
    tabs = [generators.random_deterministic(6, 2, seed=100 + k, terminal_rate=0.1) for k in range(64)]
    model = load(ctx, tabs)
    roots = np.arange(n)
    # (7 * i) % 64 alone repeats with period 64, and the grid is a multiple of 64 on a device of 256 compute units: roots r and
    # r + grid of one workgroup would share a table.  The pass number i // grid moves the second and third root of a workgroup on
    model_index, local = (7 * roots + roots // grid) % 64, (5 * roots + roots // 64) % 6
    assert all(model_index[r] != model_index[r + grid] for r in range(n - grid))
    always = {n - 1} | {r + k for r in range(4) for k in (0, grid)}
    spread = np.random.default_rng(5).choice(n, size=128 - len(always), replace=False).tolist()
    sample = sorted(always | set(spread))
    check(ctx, p, tabs, model, model_index, local, sample, form, tree_roots=(0,))
    model.close()


# ------------------------------------------------------------------------------------------- 3. slots and the highway shape
@pytest.fixture(scope="module")
def highway_tables():
    return [generators.highway_shaped(3, 4, 10, collision_rate=0.03 + 0.01 * (k % 5), seed=7000 + k) for k in range(512)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("plan", [pytest.param(KL_UNIFORM, id="olop"), pytest.param(BRUE_60, id="brue")])
def test_65536_roots_on_512_highway_tables(ctx, monkeypatch, highway_tables, plan, form):
    monkeypatch.setenv("MP_EACH_MODEL", form)
    p = sized(plan)
    n = 65536
    model = load(ctx, highway_tables)
    roots = np.arange(n)
    model_index, local = roots % 512, (roots * 37 + roots // 512) % 120
    keep = keeps_trees(p, 5, n)
    assert keep == (p["kind"] == "brue")        # OLOP's trees at this budget exceed the kept workspace: slots per workgroup
    sample = sorted({0, n - 1} | set(np.random.default_rng(6).choice(n, size=62, replace=False).tolist()))
    check(ctx, p, highway_tables, model, model_index, local, sample, form, tree_roots=(0,))
    model.close()


# ------------------------------------------------------------------------------------------------------ 4. the LDS boundary
@pytest.mark.parametrize("plan", [pytest.param(dict(kind="olop", budget=30, gamma=0.8, kl=True, continuation="uniform"), id="olop"),
                                  pytest.param(dict(kind="brue", budget=30, gamma=0.8), id="brue")])
def test_the_largest_table_in_lds_and_the_next_one(ctx, monkeypatch, plan):
    """No knob: the largest S_each at |A| = 3 that takes the LDS form by default (the measured footprint) and the next one.
    MP_EACH_MODEL=lds: the largest that fits a compute unit's LDS -- a launch with more than 64 KiB of dynamic LDS -- and the next
    one, where the knob is ignored."""
    p = sized(plan)
    cus = ctx.device_info()["n_cu"]
    info = native.each_form_info(p["kind"], 1, 3, p["horizon"], 5, cus)
    arrays = info["lds_bytes"] - 48
    for knob, limit in ((None, info["default_limit"]), ("lds", info["fit_limit"])):
        if knob:
            monkeypatch.setenv("MP_EACH_MODEL", knob)
        else:
            monkeypatch.delenv("MP_EACH_MODEL", raising=False)
        s_max = (limit - arrays) // 48
        for s_each, form in ((s_max, "lds"), (s_max + 1, "global")):
            assert native.each_form_info(p["kind"], s_each, 3, p["horizon"], 5, cus)["lds"] == (form == "lds")
            tabs = [generators.random_deterministic(s_each, 3, seed=300 + k, terminal_rate=0.05) for k in range(2)]
            model = load(ctx, tabs)
            check(ctx, p, tabs, model, [1, 0, 1, 1, 0], [s_each - 1, 0, 17, s_each // 2, s_each - 2], range(5), form, tree_roots=(0,))
            model.close()


# --------------------------------------------------------------------------------------------------------------- 5. |A| = 70
@pytest.mark.parametrize("form", FORMS)
def test_70_actions_with_availability_and_a_listing_order(ctx, monkeypatch, form):
    """The 64-wide chunks of OLOP's expansion -- availability ballot, listing order, the rank of the "zeros" action -- read
    from the root's records in LDS; BRUE draws over all 70."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    S, A = 10, 70
    tabs = [generators.random_deterministic(S, A, seed=501 + k, terminal_rate=0.1) for k in range(2)]
    avail = [generators.random_available(S, A, seed=510 + k, rate=0.2) for k in range(2)]
    for av in avail:
        av[:, 0] = True
    order = list(np.random.default_rng(503).permutation(A))
    order.remove(0)
    order.insert(66, 0)                  # action 0 is listed 67th: its device label is past the first chunk
    order = [int(a) for a in order]
    model = load(ctx, tabs, avail, order)
    model_index, local = [1, 0, 0, 1, 1, 0], [0, 3, 9, 5, 9, 0]
    for cont in ("zeros", "uniform"):
        p = sized(dict(kind="olop", budget=400, gamma=0.9, kl=True, continuation=cont))
        check(ctx, p, tabs, model, model_index, local, range(6), form, tree_roots=(0, 5), available=avail, order=order)
    model.close()
    plain = load(ctx, tabs)
    check(ctx, sized(dict(kind="brue", budget=200, gamma=0.8)), tabs, plain, model_index, local, range(6), form, tree_roots=(0, 5))
    plain.close()


# ------------------------------------------------------------------------------------------ 6. update_tables between two plans
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("plan", [pytest.param(KL_UNIFORM, id="olop"), pytest.param(BRUE_60, id="brue")])
def test_update_tables_between_two_plans(ctx, monkeypatch, plan, form):
    monkeypatch.setenv("MP_EACH_MODEL", form)
    p = sized(plan)
    tabs = [generators.random_deterministic(12, 3, seed=40 + k, terminal_rate=0.2) for k in range(4)]
    model = load(ctx, tabs)
    model_index, local = [3, 0, 3, 1, 2, 0, 1], [0, 5, 11, 7, 2, 9, 4]
    first, rng0, _ = check(ctx, p, tabs, model, model_index, local, range(7), form)
    new = list(tabs)
    new[1] = generators.random_deterministic(12, 3, seed=99, terminal_rate=0.2)
    t, r, term = stack([new[1]])
    model.update_tables(1, t, r, term)
    second, rng1, _ = check(ctx, p, new, model, model_index, local, range(7), form)       # (same seeds: the saved records)
    assert np.array_equal(rng0, rng1)
    others = [i for i, m in enumerate(model_index) if m != 1]
    for k in ("plans", "env_steps", "status"):
        assert np.array_equal(first[k][others], second[k][others]), k
    assert np.array_equal(bits(first["root_value"][others]), bits(second["root_value"][others]))
    model.close()


# -------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(ctx, monkeypatch):
    monkeypatch.delenv("MP_EACH_MODEL", raising=False)
    po, pb = sized(KL_UNIFORM), sized(BRUE_60)
    rng = native.seed_sequence_states([3], 0, 2)
    dense = generators.random_stochastic(8, 2, seed=1)
    sparse = generators.random_sparse(8, 2, 2, seed=2)
    models = [ctx.load_dense(dense["transition"], dense["reward"], dense["terminal"]),
              ctx.load_sparse(sparse["transition"], sparse["next"], sparse["reward"], sparse["terminal"])]
    for model in models:
        for p in (po, pb):
            with pytest.raises(native.NativeError) as e:
                device_plan(ctx, model, p, [0, 0], [1, 2], rng.copy())
            assert e.value.code == native.MP_ERR_MODE
        model.close()
    tabs = [generators.random_deterministic(12, 3, seed=60 + k) for k in range(3)]
    tabs[1]["reward"] = tabs[1]["reward"] * 3.0 - 1.0          # one MDP whose rewards leave [0, 1]
    model = load(ctx, tabs)
    for p in (po, pb):
        for bad in ([0, 3], [-1, 0]):                           # model_index outside [0, N) in a host array
            with pytest.raises(native.NativeError) as e:
                device_plan(ctx, model, p, bad, [1, 2], rng.copy())
            assert e.value.code == native.MP_ERR_ARG
        with pytest.raises(native.NativeError) as e:            # a local state outside [0, S_each)
            device_plan(ctx, model, p, [0, 1], [1, 12], rng.copy())
        assert e.value.code == native.MP_ERR_ARG
    rng3 = native.seed_sequence_states([4], 0, 3)
    out = device_plan(ctx, model, po, [0, 1, 2], [1, 2, 3], rng3)
    assert out["status"].tolist() == [native.MP_OK, native.MP_ERR_REWARD_RANGE, native.MP_OK]
    for i in (0, 2):
        res, rng_after = restated(po, tabs[i], [1, 2, 3][i], native.seed_sequence_states([4], 0, 3)[i])
        assert_root(po, out, rng3, i, res, rng_after)
    model.close()
