"""MDP-GapE with transition bounds on a batch model with one MDP per root (mp_gape_plan_stochastic_models, the kernel forms of
mp_gape_stoch_each_form_names) against the unmodified reference's per-episode agents (tests/golden/per_episode_gape_stoch.npz),
against mp_gape_plan_stochastic on one table and mp_gape_plan_models at K = 1, and against the test-side restatement
(tests/gape_stoch_restatement.py) run on each root's OWN table alone; then PerEpisodeEvaluation with ``kind="gape_stoch"``.

Both forms are forced in turn and the form taken is asserted.  Tolerances are those of tests/test_gpu_gape_stoch.py: every
discrete output exactly, bounds within 1e-12 / (1 - gamma) (the device's log and exp); against the other entry points everything
bit for bit, the arithmetic being the same.  The sweep leaves out the plans whose margin is 1e-9 or less under the rule of
tests/gape_cases.py: 0 of its 95 (tests/test_each_gape_stoch_host.py counts them on the CPU)."""
import functools

import numpy as np
import pytest

from rl_agents_amd import native
from tests import gape_restatement as gr
from tests import gape_stoch_cases as gsc
from tests import gape_stoch_each_cases as ge
from tests import gape_stoch_restatement as gs
from tests.gape_cases import MARGIN, SKIP_CAP, records
from tests.helpers import assert_form, generator_from
from tests.test_each_gape_stoch_host import GOLDEN, fixture_case
from tests.test_gpu_gape_stoch import BOUND_TOL, BOUNDS, EXACT

pytestmark = pytest.mark.gpu

FORMS = ["lds", "global"]
RESULTS = ("plans", "plan_len", "episodes_run", "env_steps", "status", "child_lower", "child_upper", "child_count", "best_challenger")


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def restated_case(i):
    """Case i of the per-root sweep and the restatement of its five plans, computed once for both forms."""
    case = ge.each_case(i)
    return case, ge.restate_each(case)


def load(ctx, tables):
    t, r, term, available, column = ge.device_tables(tables)
    model = ctx.load_table_batch(t, r, term, done_rule="next" if bool(tables[0]["done_on_next"]) else "source")
    if not available.all():
        model.set_available(available)
    return model, column


def plan(ctx, model, column, case, model_index, local, rng, count=None):
    """One mp_gape_plan_stochastic_models call (``model_index`` None: mp_gape_plan_stochastic) with the config of a golden-layout
    case."""
    thr, tthr = gsc.tables(case)
    run = (int(case["episodes"]), int(case["horizon"]), int(case["max_next_states_count"] if count is None else count),
           float(case["gamma"]), float(case["accuracy"]), str(case["continuation"]) == "uniform", len(column), column, thr, tthr,
           gr.value_init(float(case["gamma"]), int(case["horizon"])), rng)
    if model_index is None:
        return ctx.gape_plan_stochastic(model, np.asarray(local, np.int32), *run)
    return ctx.gape_plan_stochastic_models(model, np.asarray(model_index, np.int32), np.asarray(local, np.int32), *run)


def globalized(tree, base):
    """A tree of LOCAL states as the export of a root on the MDP that starts at ``base`` serves it: the states, and the keys of the
    decision nodes that stand for an observed state, shifted; placeholders (state -1, key < 0) as they are."""
    out = dict(tree)
    out["state"] = np.where(tree["state"] >= 0, tree["state"] + base, tree["state"]).astype(np.int32)
    observed = (tree["kind"] == 0) & (tree["parent"] >= 0) & (tree["action"] >= 0)
    out["action"] = np.where(observed, tree["action"] + base, tree["action"]).astype(np.int32)
    return out


def local_tree(ctx, root, base, order):
    """The exported tree with LOCAL states and the chance nodes' columns as the environment's actions."""
    tree = ctx.gape_stoch_tree(root)
    chance = tree["kind"] == 1
    assert ((tree["state"] >= base) | (tree["state"] == -1)).all()
    back = globalized(tree, -base)
    back["action"] = np.where(chance, np.asarray(order)[np.clip(tree["action"], 0, len(order) - 1)], back["action"]).astype(np.int32)
    return back


def assert_tree(tree, ref, gamma, name):
    for k in EXACT + ("state",):
        assert np.array_equal(tree[k], ref[k]), (name, k)
    for k in BOUNDS:
        err = np.abs(np.asarray(tree[k]) - np.asarray(ref[k]))
        assert np.all(err <= BOUND_TOL / (1 - gamma)), (name, k, err.max())


def assert_root(out, rng, i, res, after, order, column, gamma, name):
    """Root i of a call (columns) against the restatement's plan on its own table (the environment's action ids)."""
    assert np.array_equal(rng[i], after), name
    assert int(out["env_steps"][i]) == res["env_steps"], name
    if res["error"]:
        assert res["error"] == "one_action" and int(out["status"][i]) == native.ERR_GAPE_NO_CHALLENGER, name
        assert int(out["plan_len"][i]) == 0 and int(out["plans"][i, 0]) == -1, name
        return
    assert int(out["status"][i]) == native.MP_OK and int(out["plan_len"][i]) == 1, name
    assert [int(order[a]) for a in out["plans"][i]] == res["plan"].tolist(), name
    assert [int(order[a]) for a in out["best_challenger"][i]] == [res["best"], res["challenger"]], name
    assert int(out["episodes_run"][i]) == res["episodes_run"], name
    arms = np.flatnonzero((res["kind"] == 1) & (res["parent"] == 0))
    cols = column[res["action"][arms]]
    assert np.array_equal(out["child_count"][i, cols], res["count"][arms]), name
    assert (np.delete(out["child_count"][i], cols) == -1).all(), name
    for key, ref in (("child_upper", "vu"), ("child_lower", "vl")):
        err = np.abs(out[key][i, cols] - res[ref][arms])
        assert np.all(err <= BOUND_TOL / (1 - gamma)), (name, key, err.max())


def form_name(form, keep=True):
    return "gape_stoch_each_" + form + ("" if keep else "_slots")


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ------------------------------------------------------------------------------------------- 1. the unmodified reference's steps
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["k2", "k3"])
def test_golden_lock_step_through_the_entry_point(ctx, z, monkeypatch, name, form):
    """load_table_batch, update_tables per step, one gape_plan_stochastic_models(live) over the live episodes."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    n, t_steps = z["transition"].shape[:2]
    s_each, n_actions = z["reward"].shape[-2:]
    gamma = float(z[name + "/gamma"])
    column = np.arange(n_actions, dtype=np.int32)
    rng = np.stack([z["{}/e{}/t0/rng_before".format(name, e)] for e in range(n)])
    model, trees, shrunk = None, 0, False
    for t in range(t_steps):
        tr, rw, term = z["transition"][:, t], z["reward"][:, t], z["terminal"][:, t].astype(np.uint8)
        if model is None:
            model = ctx.load_table_batch(tr, rw, term)
        else:
            model.update_tables(0, tr, rw, term)
        live = np.array([e for e in range(n) if t < int(z["{}/e{}/n_steps".format(name, e)])], np.int32)
        shrunk |= len(live) < n
        states = np.array([z["{}/e{}/states".format(name, e)][t] for e in live], np.int32)
        live_rng = np.ascontiguousarray(rng[live])
        out = plan(ctx, model, column, fixture_case(z, name, 0, t), live, states, live_rng)
        assert_form(ctx, form_name(form))
        rng[live] = live_rng
        for k, e in enumerate(live):
            p = "{}/e{}/t{}".format(name, e, t)
            assert int(out["status"][k]) == native.MP_OK and out["plans"][k].tolist() == z[p + "/plan"].tolist(), p
            np.testing.assert_array_equal(rng[e], z[p + "/rng_after"], err_msg=p)
            assert int(out["episodes_run"][k]) == int(z[p + "/episodes_run"]) and int(out["env_steps"][k]) == int(z[p + "/env_steps"]), p
            arms = z[p + "/arm_action"]
            assert np.array_equal(out["child_count"][k, arms], z[p + "/arm_count"]), p
            assert (np.delete(out["child_count"][k], arms) == -1).all(), p
            for key, ref in (("child_lower", "arm_lower"), ("child_upper", "arm_upper")):
                err = np.abs(out[key][k, arms] - z[p + "/" + ref])
                assert np.all(err <= BOUND_TOL / (1 - gamma)), (p, key, err.max())
            if p + "/tree/parent" in z.files:
                tree = local_tree(ctx, k, int(e) * s_each, column)
                ref = {key: z[p + "/tree/" + key] for key in EXACT + BOUNDS}
                for key in EXACT:
                    assert np.array_equal(tree[key], ref[key]), (p, key)
                for key in BOUNDS:
                    assert np.all(np.abs(tree[key] - ref[key]) <= BOUND_TOL / (1 - gamma)), (p, key)
                trees += 1
    # ("k2" holds the episode that ends by its own actions; in "k3" every episode runs its three steps)
    assert trees == 1 and shrunk == (name == "k2")
    model.close()


# ------------------------------------------------------------------------------- 2. equal to the entry points on one table
@pytest.mark.parametrize("form", FORMS)
def test_copies_of_one_table_equal_the_plain_entry_points(ctx, monkeypatch, form):
    """4 copies of a masked table, 6 roots, K = 2: every result, the records and every tree array are mp_gape_plan_stochastic's on
    that table alone; at K = 1 the same call is also mp_gape_plan_models', bit for bit."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    case, _ = restated_case(3)                                   # masked, listing order permuted
    one = dict(case["tables"][2], max_next_states_count=2)
    assert not one["available"].all()
    copies = 4
    model, column = load(ctx, [one] * copies)
    s_each = one["mdp/reward"].shape[0]
    model_index = np.asarray([3, 0, 2, 2, 1, 0], np.int32)
    local = (np.arange(6) * 11 % s_each).astype(np.int32)
    rng0 = records(np.random.default_rng(5), 6)
    plain, _ = load(ctx, [one])                                  # (a batch of one MDP is a single table to the plain entry)
    for count in (2, 1):
        rng = rng0.copy()
        out = plan(ctx, model, column, one, model_index, local, rng, count)
        assert_form(ctx, form_name(form))
        trees = [ctx.gape_stoch_tree(i) for i in range(6)]
        rng1 = rng0.copy()
        ref = plan(ctx, plain, column, one, None, local, rng1, count)
        assert_form(ctx, "gape_stoch_table")
        for k in RESULTS:
            assert np.array_equal(bits(out[k]), bits(ref[k])), (count, k)
        assert np.array_equal(rng, rng1), count
        assert (out["status"] == native.MP_OK).any()
        for i in range(6):
            want = globalized(ctx.gape_stoch_tree(i), int(model_index[i]) * s_each)
            assert set(want) == set(trees[i])
            for k in want:
                assert np.array_equal(bits(trees[i][k]), bits(want[k])), (count, i, k)
        if count == 1:
            # mp_gape_plan_models: the header's promise for the plain entries, here for the batch entries
            rng2 = rng0.copy()
            thr, _ = gsc.tables(one)
            old = ctx.gape_plan(model, local, int(one["episodes"]), int(one["horizon"]), float(one["gamma"]), float(one["accuracy"]),
                                str(one["continuation"]) == "uniform", len(column), column, thr,
                                gr.value_init(float(one["gamma"]), int(one["horizon"])), rng2, model_index=model_index)
            assert ctx.last_kernel_variant() in native.gape_each_form_names()
            for k in RESULTS:
                assert np.array_equal(bits(out[k]), bits(old[k])), ("gape_plan_models", k)
            assert np.array_equal(rng, rng2)
            for i in range(6):
                bfs = dict(gr.as_bfs(ctx.gape_tree(i)))
                for k in bfs:
                    assert np.array_equal(bits(trees[i][k]), bits(bfs[k])), ("gape_plan_models", i, k)
    plain.close()
    model.close()


# ------------------------------------------------------------------------------------------ 3. the sweep on each root's own table
@pytest.mark.parametrize("form", FORMS)
def test_sweep_against_the_restatement(ctx, monkeypatch, form):
    monkeypatch.setenv("MP_EACH_MODEL", form)
    plans = skipped = errors = 0
    for i in range(ge.N_CASES):
        case, restated = restated_case(i)
        base = case["base"]
        gamma, order = float(base["gamma"]), base["order"]
        s_each, n_actions = base["mdp/reward"].shape
        model, column = load(ctx, case["tables"])
        rng = case["rng"].copy()
        out = plan(ctx, model, column, base, case["model_index"], case["local"], rng)
        info = native.gape_stoch_each_form_info(s_each, n_actions, int(base["horizon"]), ge.TABLES, ctx.device_info()["n_cu"])
        assert info["lds"] == (form == "lds")                    # every table of the sweep fits a compute unit's LDS
        assert_form(ctx, form_name(form))
        for k, (res, after, m) in enumerate(restated):
            plans += 1
            if not m > MARGIN:
                skipped += 1
                continue
            assert_root(out, rng, k, res, after, order, column, gamma, (i, k))
            errors += bool(res["error"])
            if not res["error"]:
                assert_tree(local_tree(ctx, k, k * s_each, order), gs.as_bfs(res), gamma, (i, k))
        model.close()
    print("per-root sweep ({}): {} plans, {} skipped for their margin, {} one-action errors".format(form, plans, skipped, errors))
    assert plans == 95 and skipped <= SKIP_CAP * plans, skipped
    assert errors >= 1


# ------------------------------------------------------------------------------------- 4. more roots than workgroups (stale LDS)
@pytest.mark.parametrize("form", FORMS)
def test_a_workgroup_reloads_the_table_of_its_next_root(ctx, monkeypatch, form):
    """Three workgroups plan two roots, at horizon 2 and 4 episodes.  First run: the two sit on different tables -- a root served
    from the previous root's copy would plan on the wrong MDP (and list the wrong actions: every table has a mask of its own).
    Second run: they sit on the same table -- the copy is skipped.  Every replica of a (table, state, record) triple must equal
    its original, which is held to the restatement on its own table."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    case, _ = restated_case(3)
    assert case["masked"]
    tables = [dict(c, horizon=2, episodes=4, accuracy=0.0, max_next_states_count=2) for c in case["tables"]]
    base = tables[0]
    gamma = float(base["gamma"])
    s_each, n_actions = base["mdp/reward"].shape
    cus = ctx.device_info()["n_cu"]
    grid = native.gape_stoch_each_form_info(s_each, n_actions, 2, 1 << 30, cus)["grid"]
    n = grid + 3
    info = native.gape_stoch_each_form_info(s_each, n_actions, 2, n, cus)
    assert info["grid"] == grid and info["lds"] == (form == "lds")
    model, column = load(ctx, tables)
    restated = [gsc.restate_plan(tables[k], int(case["local"][k]), case["rng"][k]) for k in range(ge.TABLES)]
    first = np.arange(grid) % ge.TABLES
    for second, what in (((first[:3] + 1) % ge.TABLES, "another table"), (first[:3], "the same table")):
        triple = np.concatenate([first, second])
        assert (triple[grid:] != triple[:3]).all() == (what == "another table")
        rng = np.ascontiguousarray(case["rng"][triple])
        out = plan(ctx, model, column, base, case["model_index"][triple], case["local"][triple], rng)
        assert_form(ctx, form_name(form))
        held = 0
        for k in range(ge.TABLES):
            res, after, seen = restated[k]
            if gsc.margin(seen) > MARGIN:
                assert_root(out, rng, k, res, after, base["order"], column, gamma, (what, k))
                held += 1
            at = np.flatnonzero(triple == k)
            for key in RESULTS:
                got = np.ascontiguousarray(np.asarray(out[key])[at]).reshape(len(at), -1).view(np.uint8)
                assert (got == got[:1]).all(), (what, k, key)
            assert (rng[at] == rng[at[:1]]).all(), (what, k)
        assert held == ge.TABLES, held                           # (checked on the CPU: no margin of the five is 1e-9 or less)
        for root in (0, grid, n - 1):                            # a first root, and the second roots of two workgroups
            original = ctx.gape_stoch_tree(int(triple[root]))
            replica = ctx.gape_stoch_tree(root)
            for key in original:
                assert np.array_equal(bits(replica[key]), bits(original[key])), (what, root, key)
    model.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. fit
def fit_tables(s_each, n_tables, seed):
    out = []
    for k in range(n_tables):
        cfg = gsc.table("deterministic", s_each, 3, 0, seed + k, 0.0)
        out.append(gsc.pack(cfg, None, None, False, [0], np.zeros((1, 6), np.uint64), horizon=3, episodes=8, gamma=0.8, accuracy=0.0,
                            continuation="uniform", threshold=gsc.LOG_TIME, max_next_states_count=2,
                            transition_threshold=gsc.DEFAULT_TRANSITION))
    return out


@pytest.mark.parametrize("form", FORMS)
def test_smallest_and_largest_tables(ctx, monkeypatch, form):
    """S_each = 1; the largest S_each at |A| = 3 whose records fit a compute unit's LDS behind path[7], and one more, where the
    forced LDS form falls back to the global one."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    cus = ctx.device_info()["n_cu"]
    s_max = (native.gape_stoch_each_form_info(1, 3, 3, 1, cus)["fit_limit"] - 32) // (3 * 16)
    for s_each, fits in ((1, True), (s_max, True), (s_max + 1, False)):
        tables = fit_tables(s_each, 3, 300 + s_each % 7)
        info = native.gape_stoch_each_form_info(s_each, 3, 3, 4, cus)
        assert (info["lds_bytes"] <= info["fit_limit"]) == fits and info["lds"] == (form == "lds" and fits)
        model, column = load(ctx, tables)
        model_index = np.asarray([2, 0, 1, 2], np.int32)
        local = np.asarray([0, s_each - 1, s_each // 2, s_each - 1], np.int32)
        rng0 = records(np.random.default_rng(s_each), 4)
        rng = rng0.copy()
        out = plan(ctx, model, column, tables[0], model_index, local, rng)
        assert_form(ctx, form_name("lds" if info["lds"] else "global"))
        compared = 0
        for i in range(4):
            res, after, seen = gsc.restate_plan(tables[model_index[i]], int(local[i]), rng0[i])
            if gsc.margin(seen) > MARGIN:
                assert_root(out, rng, i, res, after, np.arange(3), column, 0.8, (s_each, i))
                assert_tree(local_tree(ctx, i, int(model_index[i]) * s_each, np.arange(3)), gs.as_bfs(res), 0.8, (s_each, i))
                compared += 1
        assert compared == 4, (s_each, compared)                 # (checked on the CPU: the smallest margin is 1.2e-5)
        model.close()


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(ctx, monkeypatch):
    from rl_agents_amd.envs import generators
    monkeypatch.delenv("MP_EACH_MODEL", raising=False)
    case, _ = restated_case(0)
    base = case["base"]
    column = np.arange(base["mdp/reward"].shape[1], dtype=np.int32)
    rng = records(np.random.default_rng(1), 2)

    def code(model, model_index, local, count=None):
        with pytest.raises(native.NativeError) as e:
            plan(ctx, model, column, base, model_index, local, rng, count)
        return e.value.code

    one = case["tables"][0]
    dense, sparse = generators.random_stochastic(8, 5, seed=1), generators.random_sparse(8, 5, 2, seed=2)
    t, r, term, _, _ = ge.device_tables(case["tables"][:2])
    others = [ctx.load_table(one["mdp/transition"], one["mdp/reward"], one["mdp/terminal"]),        # a single table
              ctx.load_dense(dense["transition"], dense["reward"], dense["terminal"]),
              ctx.load_sparse(sparse["transition"], sparse["next"], sparse["reward"], sparse["terminal"]),
              ctx.load_joint(t, r, term),
              ctx.load_joint_batch(np.stack([t, t]), np.stack([r, r]), np.stack([term, term]))]
    for model in others:
        assert code(model, [0, 0], [1, 2]) == native.MP_ERR_MODE
        model.close()
    model, _ = load(ctx, case["tables"])
    s_each = base["mdp/reward"].shape[0]
    for bad in ([0, ge.TABLES], [-1, 0]):                        # model_index outside [0, N) in a host array
        assert code(model, bad, [1, 2]) == native.MP_ERR_ARG
    for bad in ([1, s_each], [-1, 2]):                           # a local state outside [0, S_each)
        assert code(model, [0, 1], bad) == native.MP_ERR_ARG
    for count in (0, 33):                                        # K outside 1..32
        assert code(model, [0, 1], [1, 2], count) == native.MP_ERR_ARG
    assert code(model, None, [1, 2]) == native.MP_ERR_MODE       # mp_gape_plan_stochastic itself keeps refusing batch models
    assert np.array_equal(rng, records(np.random.default_rng(1), 2))
    # and the call the refusals surround goes through, on the default form: the global one
    out = plan(ctx, model, column, base, [0, 1], [1, 2], rng)
    assert_form(ctx, form_name("global"))
    assert out["status"].shape == (2,) and not np.array_equal(rng, records(np.random.default_rng(1), 2))
    model.close()


# ---------------------------------------------------------------------------------------------------------------- 7. the loop
def scheduled_envs(z, spoil=None):
    from rl_agents_amd.envs import ScheduledTableEnv
    envs = []
    for e in range(z["transition"].shape[0]):
        tables = [dict(mode="deterministic", transition=z["transition"][e, t], reward=z["reward"][e, t].copy(),
                       terminal=z["terminal"][e, t]) for t in range(z["transition"].shape[1])]
        if spoil is not None and e == spoil[0]:
            tables[spoil[1]]["reward"][:] = 1.5
        envs.append(ScheduledTableEnv(tables, state=int(z["s0"][e])))
    return envs


def gape_config(z, name):
    return dict(horizon=int(z[name + "/horizon"]), episodes=int(z[name + "/episodes"]), gamma=float(z[name + "/gamma"]),
                accuracy=float(z[name + "/accuracy"]), confidence=float(z[name + "/confidence"]), budget=int(z[name + "/budget"]),
                continuation_type=str(z[name + "/continuation"]), max_next_states_count=int(z[name + "/max_next_states_count"]),
                upper_bound=dict(type="kullback-leibler", threshold=str(z[name + "/threshold"]),
                                 transition_threshold=str(z[name + "/transition_threshold"])))


@pytest.mark.parametrize("name", ["k2", "k3"])
def test_golden_per_episode_evaluation(z, name):
    from rl_agents_amd.agents.tree_search.mdp_gape import PerEpisodeStochasticMDPGapEAgent, StochasticMDPGapEAgent
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    envs = scheduled_envs(z)
    agent = PerEpisodeStochasticMDPGapEAgent(envs[0], gape_config(z, name))
    with pytest.raises(NotImplementedError, match="no kind that plans PerEpisodeStochasticMDPGapE"):
        PerEpisodeEvaluation(envs, agent, sim_seed=100, max_steps=3)
    with pytest.raises(ValueError, match="StochasticMDPGapE offers"):
        PerEpisodeEvaluation(envs, StochasticMDPGapEAgent(envs[0], gape_config(z, name)), sim_seed=100, max_steps=3, kind="gape_stoch")
    ev = PerEpisodeEvaluation(envs, agent, sim_seed=100, max_steps=3, kind="gape_stoch")
    out = ev.run()
    assert ev.ctx.last_kernel_variant() in native.gape_stoch_each_form_names()
    n = len(envs)
    n_steps = [int(z["{}/e{}/n_steps".format(name, e)]) for e in range(n)]
    assert out["lengths"].tolist() == n_steps and min(n_steps) == (2 if name == "k2" else 3)
    total = 0
    for e in range(n):
        for t in range(n_steps[e]):
            p = "{}/e{}/t{}".format(name, e, t)
            assert int(out["actions"][e, t]) == int(z[p + "/plan"][0]), p
            total += int(z[p + "/env_steps"])
        np.testing.assert_array_equal(ev.rng[e], z["{}/e{}/t{}/rng_after".format(name, e, n_steps[e] - 1)])
    assert out["planner_env_steps"] == total and out["uploads"] == sum(n_steps)
    ev.close()


def highway_envs(n, seed0=500):
    from rl_agents_amd.envs import ChangingHighwayEnv
    return [ChangingHighwayEnv(3, 4, 10, table_seed=seed0 + 20 * i, state=((i % 3) * 4 + (i % 4)) * 10,
                               collision_rate=0.03 + 0.02 * (i % 4)) for i in range(n)]


def test_changing_highway_batch_equals_sequential_agents():
    """highway-env's surface (restricted action sets listed IDLE first) with a table re-drawn after every step, six
    environments: the batch == six sequential StochasticMDPGapEAgent loops of this package, action for action."""
    from rl_agents_amd.agents.tree_search.mdp_gape import PerEpisodeStochasticMDPGapEAgent, StochasticMDPGapEAgent
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    from tests.test_gpu_per_episode_olop_brue import _sequential
    n, steps = 6, 4
    cfg = dict(horizon=3, episodes=12, gamma=0.8, accuracy=0.1, max_next_states_count=2,
               upper_bound=dict(type="kullback-leibler", threshold=gsc.LOG_TIME))
    batch_envs = highway_envs(n)
    ev = PerEpisodeEvaluation(batch_envs, PerEpisodeStochasticMDPGapEAgent(batch_envs[0], dict(cfg)), sim_seed=7, max_steps=steps,
                              kind="gape_stoch")
    out = ev.run()
    assert ev.ctx.last_kernel_variant() in native.gape_stoch_each_form_names()
    acts, returns = _sequential(highway_envs(n), lambda env: StochasticMDPGapEAgent(env, dict(cfg)), 7, steps)
    np.testing.assert_array_equal(out["actions"], acts)
    assert np.array_equal(out["returns"], returns)
    assert (out["actions"][:, 0] >= 0).all() and out["uploads"] >= n
    ev.close()


def test_a_reward_out_of_range_raises_with_the_draws_written_back(z):
    """Episode 2's table of the second step pays 1.5: the planner's ValueError, and every live episode's generator record is what
    the device left -- for the other episodes the reference's record after that step's plan."""
    from rl_agents_amd.agents.tree_search.mdp_gape import PerEpisodeStochasticMDPGapEAgent
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    envs = scheduled_envs(z, spoil=(2, 1))
    ev = PerEpisodeEvaluation(envs, PerEpisodeStochasticMDPGapEAgent(envs[0], gape_config(z, "k2")), sim_seed=100, max_steps=3,
                              kind="gape_stoch")
    with pytest.raises(ValueError, match="rewards are normalized"):
        ev.run()
    assert int(z["k2/e2/n_steps"]) >= 2
    for e in range(len(envs)):
        if e != 2 and int(z["k2/e{}/n_steps".format(e)]) >= 2:
            np.testing.assert_array_equal(ev.rng[e], z["k2/e{}/t1/rng_after".format(e)])
    one_draw = generator_from(z["k2/e2/t1/rng_before"])
    one_draw.integers(2 ** 30)                                   # the failing plan's first episode drew its seed, then stepped
    np.testing.assert_array_equal(ev.rng[2], native.rng_state_from_generator(one_draw))
    ev.close()
