"""MDP-GapE on the device (mp_gape_plan, rl_agents_amd/csrc/gape.hip) against the restatement (tests/gape_restatement.py) beyond
the fixed inputs of tests/test_gpu_gape.py: the sweep of tests/gape_cases.py (96 drawn cases and 5 hand-made ones, 2 roots each:
masks, listing orders, both done rules and continuations, horizons 1 .. 70, up to 150 actions), kept trees of more roots than
workgroups, and the root's best-arm identification with its arms in the second and third chunk of 64 lanes.

tests/test_gape_host.py checks on the CPU what the sweep contains and that at most 5 % of its plans are too close to call.
Measured with the restatement alone: 202 plans in 3.1 s; 7 of them (3.5 %) compare two values 1e-9 or less apart and are
skipped here, 2 are roots with one listed action (the reference raises), 33 stop early and 167 run all ``episodes + 2``.

The tolerances are those of tests/test_gpu_gape.py (EXACT, BOUNDS, BOUND_TOL / (1 - gamma), assert_tree): nothing new."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from tests import gape_cases as gc
from tests.helpers import assert_form
from tests.test_gape_host import GAPE_AGENT
from tests.test_gpu_gape import BOUND_TOL, SMALL, assert_tree, small_env
from tests.test_gpu_olop import golden_env

pytestmark = pytest.mark.gpu


def agent_of(case):
    env = golden_env(dict(case, s0=int(case["roots"][0])))
    cfg = dict(gamma=float(case["gamma"]), episodes=int(case["episodes"]), horizon=int(case["horizon"]),
               accuracy=float(case["accuracy"]), confidence=float(case["confidence"]), continuation_type=str(case["continuation"]),
               upper_bound=dict(type="kullback-leibler", threshold=str(case["threshold"])))
    return env, agent_factory(env, dict(cfg, __class__=GAPE_AGENT))


def device_tree(ctx, root, order):
    """The exported tree with the chance nodes' columns as the environment's actions."""
    tree = ctx.gape_tree(root)
    tree["action"] = np.where(tree["kind"] == 1, order[np.clip(tree["action"], 0, len(order) - 1)], tree["action"]).astype(np.int32)
    return tree


def assert_plan(out, i, res, rng_after, rng, gamma, name):
    """Root ``i`` of a plan_batch result (actions as the environment's) against the restatement's plan."""
    assert int(out["status"][i]) == native.MP_OK and int(out["plan_len"][i]) == 1, name
    assert out["plans"][i].tolist() == res["plan"].tolist(), name
    assert out["best_challenger"][i].tolist() == [res["best"], res["challenger"]], name
    assert int(out["episodes_run"][i]) == res["episodes_run"] and int(out["env_steps"][i]) == res["env_steps"], name
    assert np.array_equal(rng[i], rng_after), name
    arms = np.flatnonzero((res["kind"] == 1) & (res["parent"] == 0))
    listed = res["action"][arms]
    assert np.array_equal(out["child_count"][i, listed], res["count"][arms]), name
    assert (np.delete(out["child_count"][i], listed) == -1).all(), name
    for key, ref in (("child_upper", "vu"), ("child_lower", "vl")):
        err = np.abs(out[key][i, listed] - res[ref][arms])
        assert np.all(err <= BOUND_TOL / (1 - gamma)), (name, key, err.max())
        assert (np.delete(out[key][i], listed) == 0).all(), name


def test_sweep_against_the_restatement():
    plans = skipped = errors = 0
    for c in range(gc.N_CASES):
        case = gc.sweep_case(c)
        restated = gc.restate_case(case)
        env, agent = agent_of(case)
        planner, gamma, order = agent.planner, float(case["gamma"]), case["order"]
        roots, rng = case["roots"].copy(), case["rng"].copy()
        failing = [res["error"] for res, _, _ in restated if res["error"]]
        assert set(failing) <= {"one_action"}, c
        plans += len(restated)
        if failing:
            # the agent raises what the reference raises, with the draws and steps of every root made; the statuses are the C ABI's
            with pytest.raises(ValueError, match="empty sequence"):
                planner.plan_batch(env, roots, rng_states=rng)
            assert_form(planner.models.ctx, "gape_global")
            assert np.array_equal(rng, np.stack([after for _, after, _ in restated])), c
            column = np.empty(len(order), np.int32)
            column[order] = np.arange(len(order))
            rng = case["rng"].copy()
            out = planner.models.ctx.gape_plan(planner.model_for(env), roots, int(case["episodes"]), int(case["horizon"]), gamma,
                                               float(case["accuracy"]), str(case["continuation"]) == "uniform", len(order), column,
                                               planner.thresholds(), planner._value_init, rng)
            for i, (res, after, seen) in enumerate(restated):
                assert np.array_equal(rng[i], after), (c, i)
                assert int(out["env_steps"][i]) == res["env_steps"], (c, i)
                if res["error"]:
                    one_draw = gc.generator_from(case["rng"][i])
                    one_draw.integers(2 ** 30)
                    assert np.array_equal(rng[i], native.rng_state_from_generator(one_draw)), (c, i)
                    assert int(out["status"][i]) == native.ERR_GAPE_NO_CHALLENGER and int(out["plan_len"][i]) == 0, (c, i)
                    assert int(out["env_steps"][i]) == 0 and int(out["plans"][i, 0]) == -1, (c, i)
                    errors += 1
                elif gc.margin(seen) > gc.MARGIN:
                    assert int(out["status"][i]) == native.MP_OK and int(order[out["plans"][i, 0]]) == int(res["plan"][0]), (c, i)
                    assert [int(order[a]) for a in out["best_challenger"][i]] == [res["best"], res["challenger"]], (c, i)
                    assert int(out["episodes_run"][i]) == res["episodes_run"], (c, i)
                    assert_tree(device_tree(planner.models.ctx, i, order), res, gamma, (c, i))
                else:
                    skipped += 1
            continue
        out = planner.plan_batch(env, roots, rng_states=rng)
        assert_form(planner.models.ctx, "gape_global")
        for i, (res, after, seen) in enumerate(restated):
            if gc.margin(seen) <= gc.MARGIN:
                skipped += 1
                continue
            assert_plan(out, i, res, after, rng, gamma, (c, i))
            assert_tree(device_tree(planner.models.ctx, i, order), res, gamma, (c, i))
    print("sweep: {} plans, {} skipped for their margin, {} roots with one listed action".format(plans, skipped, errors))
    assert plans == gc.N_CASES * gc.ROOTS and errors >= 1
    assert skipped <= gc.SKIP_CAP * plans, skipped


def test_kept_trees_with_more_roots_than_workgroups():
    """10 000 roots of 49 records: every tree is kept (gape_global) and a workgroup plans a second root after its first, which
    has to start from a fresh root record, path and counters."""
    cfg = dict(horizon=2, episodes=6, gamma=0.8, accuracy=1.4)       # (5 of the 37 roots compared stop before episode 8)
    env = small_env()
    agent = agent_factory(env, dict(cfg, __class__=GAPE_AGENT, upper_bound=dict(type="kullback-leibler", threshold=gc.LOG_TIME)))
    agent.seed(17)
    ctx = agent.planner.models.ctx
    n, grid = 10000, ctx.device_info()["n_cu"] * 32                # the resident workgroups of each_form_global
    assert grid + 1 < n, "more roots than workgroups is what this test is about"
    roots = (np.arange(n) * 7 % 12).astype(np.int32)
    rng = agent.planner.batch_rng_states(n)
    rng0 = rng.copy()
    out = agent.planner.plan_batch(env, roots, rng_states=rng)
    assert_form(ctx, "gape_global")
    assert (out["status"] == native.MP_OK).all()
    case = gc.pack(SMALL, None, None, False, roots[:1], rng0[:1], continuation="uniform", threshold=gc.LOG_TIME, **cfg)
    thr = gc.thresholds(case)
    sample = sorted({0, grid - 1, grid, grid + 1, n - 1} | {int(x) for x in np.linspace(1, n - 2, 32)})
    stopped_early = 0
    for i in sample:
        res, after, seen = gc.restate_plan(case, int(roots[i]), rng0[i], thr)
        assert gc.margin(seen) > gc.MARGIN, i
        assert_plan(out, i, res, after, rng, cfg["gamma"], i)
        assert_tree(ctx.gape_tree(i), res, cfg["gamma"], i)
        stopped_early += res["episodes_run"] < cfg["episodes"] + 2
    assert 0 < stopped_early < len(sample)


@pytest.mark.parametrize("k", sorted(gc.CHUNK_PAIRS))
def test_root_identification_in_later_chunks(k):
    """The restatement first (the arms ARE where the case means them to be, ties included), then the device against it."""
    case = gc.later_chunk_case(k)
    (res, after, seen), = gc.restate_case(case)
    lo, hi = gc.CHUNK_PAIRS[k]
    arms = np.asarray([v for kind, v in seen if kind == "arms"], np.int64)     # best, challenger, selected, top 1, top 2
    for first in (64, 128)[:2 if k > 128 else 1]:
        assert (arms[:, [0, 1, 3, 4]] >= first).any(axis=0).all(), (first, (arms >= first).sum(axis=0))
    kinds = [kind for kind, _ in seen]
    floor = 64 if k > 128 else 1            # ties over two chunks whose winner is not arm 0: in a later chunk where there are three
    ties_won_by_the_lower = {"gaps": 0, "challenger": 0}
    for at in np.flatnonzero(np.asarray(kinds) == "arms"):
        best, challenger = int(seen[at][1][0]), int(seen[at][1][1])
        assert kinds[at - 3:at] == ["gaps", "challenger", "widths"]
        for kind, values, winner, skipped in (("gaps", seen[at - 3][1], best, None), ("challenger", seen[at - 2][1], challenger, best)):
            tied = gc.tied_positions(values, skipped, lowest=kind == "gaps")
            assert tied[0] == winner
            ties_won_by_the_lower[kind] += tied[0] // 64 != tied[-1] // 64 and tied[0] >= floor
    assert min(ties_won_by_the_lower.values()) > 0, ties_won_by_the_lower
    assert res["error"] is None and res["vu"][1 + lo] == res["vu"][1 + hi] and res["vl"][1 + lo] == res["vl"][1 + hi]
    assert gc.margin(seen) > gc.MARGIN
    env, agent = agent_of(case)
    rng = case["rng"].copy()
    out = agent.planner.plan_batch(env, case["roots"], rng_states=rng)
    assert_form(agent.planner.models.ctx, "gape_global")
    assert_plan(out, 0, res, after, rng, float(case["gamma"]), k)
    assert_tree(agent.planner.models.ctx.gape_tree(0), res, float(case["gamma"]), k)
