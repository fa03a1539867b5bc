"""MDP-GapE with transition bounds on the device (mp_gape_plan_stochastic) against the restatement
(tests/gape_stoch_restatement.py) beyond the golden inputs: the sweep of tests/gape_stoch_cases.py (57 drawn cases and 3
hand-made ones: the three kinds of model, K 1 .. 6 and 32, masks, listing orders, both done rules and continuations, horizons
1 .. 5 and 20, up to 70 actions, plans that run out of placeholders), trees included, kept trees of more roots than
workgroups, and a batch whose trees pass 1 GiB: the ``_slots`` form, a slot per workgroup re-used round after round.

tests/test_gape_stoch_host.py checks on the CPU what the sweep contains and that at most 5 % of its plans are too close to call
(measured with the restatement alone: none of the 60 is).  The tolerances are those of tests/test_gpu_gape_stoch.py."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from tests import gape_stoch_cases as gc
from tests import gape_stoch_restatement as gs
from tests.helpers import assert_form
from tests.test_gape_stoch_host import STOCH_AGENT, case_agent
from tests.test_gpu_gape_stoch import BOUND_TOL, FORM, SMALL, SMALL_CFG, assert_tree, small_env

pytestmark = pytest.mark.gpu

STATUS = {"placeholders": native.ERR_GAPE_PLACEHOLDERS, "one_action": native.ERR_GAPE_NO_CHALLENGER}


def device_tree(ctx, root, order):
    """The exported tree with the chance nodes' columns as the environment's actions."""
    tree = ctx.gape_stoch_tree(root)
    tree["action"] = np.where(tree["kind"] == 1, order[np.clip(tree["action"], 0, len(order) - 1)], tree["action"]).astype(np.int32)
    return tree


def assert_plan(out, i, res, rng_after, rng, gamma, order, name):
    """Root ``i`` of a C-ABI result (actions as columns of the model) against the restatement's plan."""
    assert int(out["status"][i]) == native.MP_OK and int(out["plan_len"][i]) == 1, name
    assert [int(order[a]) for a in out["plans"][i]] == res["plan"].tolist(), name
    assert [int(order[a]) for a in out["best_challenger"][i]] == [res["best"], res["challenger"]], name
    assert int(out["episodes_run"][i]) == res["episodes_run"] and int(out["env_steps"][i]) == res["env_steps"], name
    assert np.array_equal(rng[i], rng_after), name
    arms = np.flatnonzero((res["kind"] == 1) & (res["parent"] == 0))
    column = np.empty(len(order), np.int64)
    column[order] = np.arange(len(order))
    listed = column[res["action"][arms]]
    assert np.array_equal(out["child_count"][i, listed], res["count"][arms]), name
    assert (np.delete(out["child_count"][i], listed) == -1).all(), name
    for key, ref in (("child_upper", "vu"), ("child_lower", "vl")):
        err = np.abs(out[key][i, listed] - res[ref][arms])
        assert np.all(err <= BOUND_TOL / (1 - gamma)), (name, key, err.max())


def plan_call(planner, env, case, roots, rng):
    return plan_call_form(planner, env, case, roots, rng, FORM[str(case["mdp/mode"])])


def plan_call_form(planner, env, case, roots, rng, form):
    order = case["order"]
    column = np.empty(len(order), np.int32)
    column[order] = np.arange(len(order))
    ctx = planner.models.ctx
    out = ctx.gape_plan_stochastic(planner.model_for(env), roots, int(case["episodes"]), int(case["horizon"]),
                                   int(case["max_next_states_count"]), float(case["gamma"]), float(case["accuracy"]),
                                   str(case["continuation"]) == "uniform", len(order), column, planner.thresholds(),
                                   planner.transition_thresholds(), planner._value_init, rng)
    assert_form(ctx, form)
    return out


def test_sweep_against_the_restatement():
    plans = skipped = 0
    errors = {"placeholders": 0, "one_action": 0}
    for c in range(gc.N_CASES):
        case = gc.sweep_case(c)
        restated = gc.restate_case(case)
        env, agent = case_agent(dict(case, s0=int(case["roots"][0]), rng_before=case["rng"][0]))
        planner, gamma, order = agent.planner, float(case["gamma"]), case["order"]
        rng = case["rng"].copy()
        out = plan_call(planner, env, case, case["roots"], rng)
        for i, (res, after, seen) in enumerate(restated):
            plans += 1
            if gc.margin(seen) <= gc.MARGIN:
                skipped += 1
                continue
            if res["error"]:
                # the steps and draws made before the reference raises, and the status that stands for what it raises
                assert int(out["status"][i]) == STATUS[res["error"]] and int(out["plan_len"][i]) == 0, (c, i)
                assert int(out["env_steps"][i]) == res["env_steps"] and np.array_equal(rng[i], after), (c, i)
                assert int(out["plans"][i, 0]) == -1, (c, i)
                errors[res["error"]] += 1
                continue
            assert_plan(out, i, res, after, rng, gamma, order, (c, i))
            assert_tree(device_tree(planner.models.ctx, i, order), gs.as_bfs(res), gamma, (c, i))
    print("sweep: {} plans, {} skipped for their margin, errors {}".format(plans, skipped, errors))
    assert plans == gc.N_CASES * gc.ROOTS and min(errors.values()) >= 1
    assert skipped <= gc.SKIP_CAP * plans, skipped


def test_kept_trees_with_more_roots_than_workgroups():
    """10 000 roots at horizon 2 and 4 episodes: every tree is kept and a workgroup plans a second root after its first, which
    has to start from a fresh root record, path, counters and clone."""
    cfg = dict(SMALL_CFG, horizon=2, episodes=4, accuracy=1.4)
    env = small_env()
    agent = agent_factory(env, dict(cfg, __class__=STOCH_AGENT, upper_bound=dict(type="kullback-leibler", threshold=gc.LOG_TIME)))
    agent.seed(17)
    planner = agent.planner
    ctx = planner.models.ctx
    n, grid = 10000, ctx.device_info()["n_cu"] * 32                # the resident workgroups of each_form_global
    assert grid + 1 < n, "more roots than workgroups is what this test is about"
    roots = (np.arange(n) * 7 % 9).astype(np.int32)
    rng = planner.batch_rng_states(n)
    rng0 = rng.copy()
    sparse = dict(SMALL, mode="sparse")
    case = gc.pack(sparse, None, None, False, roots, rng0, continuation="uniform", threshold=gc.LOG_TIME,
                   transition_threshold=gc.DEFAULT_TRANSITION, max_next_states_count=cfg["max_next_states_count"],
                   horizon=cfg["horizon"], episodes=cfg["episodes"], gamma=cfg["gamma"], accuracy=cfg["accuracy"])
    out = plan_call(planner, env, case, roots, rng)
    assert ctx.last_kernel_variant() == "gape_stoch_sparse"        # kept trees, not slots
    assert (out["status"] == native.MP_OK).all()
    both = gc.tables(case)
    sample = sorted({0, grid - 1, grid, grid + 1, n - 1} | {int(x) for x in np.linspace(1, n - 2, 32)})
    compared = 0
    for i in sample:
        res, after, seen = gc.restate_plan(case, int(roots[i]), rng0[i], both)
        if gc.margin(seen) <= gc.MARGIN:
            continue
        assert_plan(out, i, res, after, rng, cfg["gamma"], case["order"], i)
        assert_tree(ctx.gape_stoch_tree(i), gs.as_bfs(res), cfg["gamma"], i)
        compared += 1
    assert compared >= len(sample) - 2, compared


def slots_batch():
    """41 000 roots of SMALL_CFG's 20 episodes x horizon 3: 334 records of 80 bytes a tree, 1.10 GB in all -- past the 1 GiB the
    workspace keeps, so the trees live in one slot per workgroup, and root 0's in a slot of its own."""
    cfg = dict(SMALL_CFG)
    env = small_env()
    agent = agent_factory(env, dict(cfg, __class__=STOCH_AGENT, upper_bound=dict(type="kullback-leibler", threshold=gc.LOG_TIME)))
    agent.seed(13)
    n = 41000
    roots = (np.arange(n) * 7 % 9).astype(np.int32)
    rng0 = agent.planner.batch_rng_states(n)
    case = gc.pack(dict(SMALL, mode="sparse"), None, None, False, roots, rng0, continuation="uniform", threshold=gc.LOG_TIME,
                   transition_threshold=gc.DEFAULT_TRANSITION, max_next_states_count=cfg["max_next_states_count"],
                   horizon=cfg["horizon"], episodes=cfg["episodes"], gamma=cfg["gamma"], accuracy=cfg["accuracy"])
    cap = 1 + (cfg["episodes"] + 2) * cfg["horizon"] * cfg["max_next_states_count"] + (1 + (cfg["episodes"] + 2) * cfg["horizon"]) * 3
    assert n * cap * 80 > 1 << 30
    return env, agent, case, roots, rng0


def slots_sample(n, grid):
    """Root 0 (its own slot), the first and last root of the workgroups' first round, roots of their second, third and last."""
    return sorted({0, 1, grid - 1, grid, grid + 1, 2 * grid + 3, 3 * grid + 5, n - 1})


def test_more_trees_than_the_workspace_keeps():
    env, agent, case, roots, rng0 = slots_batch()
    planner, gamma = agent.planner, float(case["gamma"])
    ctx = planner.models.ctx
    n, grid = len(roots), ctx.device_info()["n_cu"] * 32
    assert 3 * grid + 5 < n
    rng = rng0.copy()
    out = plan_call_form(planner, env, case, roots, rng, "gape_stoch_sparse_slots")
    assert (out["status"] == native.MP_OK).all()
    both = gc.tables(case)
    for i in slots_sample(n, grid):
        res, after, seen = gc.restate_plan(case, int(roots[i]), rng0[i], both)
        assert gc.margin(seen) > gc.MARGIN, i               # (tests/test_gape_stoch_host.py holds the sample to this on the CPU)
        assert_plan(out, i, res, after, rng, gamma, case["order"], i)
        if i == 0:
            assert_tree(ctx.gape_stoch_tree(0), gs.as_bfs(res), gamma, i)      # the one tree that is kept
    with pytest.raises(native.NativeError, match="only root 0's was kept"):
        ctx.gape_stoch_tree(1)
    # a later round of a workgroup starts from a clean slot: the same roots alone (kept trees) give the same results
    late = np.asarray([i for i in slots_sample(n, grid) if i >= grid])
    rng_late = rng0[late].copy()
    alone = plan_call_form(planner, env, case, roots[late], rng_late, "gape_stoch_sparse")
    for k in ("plans", "episodes_run", "env_steps", "child_lower", "child_upper", "child_count", "best_challenger"):
        assert np.array_equal(alone[k], out[k][late]), k
    assert np.array_equal(rng_late, rng[late])
