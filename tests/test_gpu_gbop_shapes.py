"""GBOP on the device (rl_agents_amd/csrc/gbop.hip) at the shapes no seed of the sweep reaches, against the restatement
(tests/gbop_cases.py builds the cases; tests/test_gbop_cases_host.py asserts on the host that each reaches its edge):

  more than 64 actions           backup_node, amax_listed, the expansion loop and the tie draw over `a0 += 64`; two chance nodes a
                                 wavefront across a chunk border; an odd listed count in a chunk; the environment's listing order
  more than 64 states a walk     the update_queue membership scan over `j0 += 64` (a state found in the second chunk: the tail
                                 cases) and its reversal into the ring
  more than 64 parents           the parents.add scan and the append of a popped node's parents, insertion order across the border
  the ring                       wrap-around at a capacity the pushes of one backup exceed; overflow per planner, sticky
  every form                     gbop_{table,dense,sparse}_global by MP_GBOP_LDS_BYTES=0 against the LDS placement by bits; the
                                 natural limit S = 1024 / 1025 without a knob

Every comparison is the sweep's (tests/test_gpu_gbop.py): status, plan with its key, generator record, env_steps and pops
exactly; the exported graph by gb.compare_listing within BOUND_TOL / (1 - gamma)."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv
from tests import gbop_cases as gc
from tests import gbop_restatement as gb
from tests.helpers import assert_form
from tests.test_gbop_host import BOUND_TOL, GBOP_AGENT
from tests.test_gpu_gbop import device_plan, load_model

pytestmark = pytest.mark.gpu

TOL = BOUND_TOL / (1 - gc.GAMMA)
RECORDED = set()          # the kernel forms this file has launched


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """Every case of this file with the restatement's answer: its CPU time is spent here, once, not in the tests."""
    return {name: gc.get_case(name) for family in ("wide", "ring", "hub", "forms", "limit") for name in gc.FAMILIES[family][0]}


def listing_in_env_ids(lst, order):
    if order is not None:
        act = lst["action"]
        lst["action"] = np.where(act >= 0, np.asarray(order)[np.maximum(act, 0)], -1).astype(np.int32)
    return lst


def run_case(ctx, monkeypatch, case, ref, placement="lds", queue_cap=None):
    """Every call of ``case`` on one kept batch of planners against the restatement's answer ``ref``.  A planner whose queue
    peak exceeds ``queue_cap`` in the restatement must answer MP_ERR_ALLOC from that call on; every other planner must equal
    the restatement.  -> (outputs of every call, exports after the last call, the planners that failed)"""
    monkeypatch.setenv("MP_GBOP_GRID", "2")
    monkeypatch.setenv("MP_GBOP_MAX_POPS", "100000")          # (no case pops 3 000 times: a plan that did not end is a status here)
    mode, t, r, nxt, av = gc.device_tables(case)
    model = load_model(ctx, mode, t, r, nxt, av)
    n, A, order = len(case["rng"]), r.shape[1], case["order"]
    handle = native.StochasticGraphBasedPlanners(ctx, model, n, case["K"], queue_cap=queue_cap)
    try:
        if queue_cap is not None:
            assert handle.info()["queue_cap"] == queue_cap
        rng = case["rng"].copy()
        failed, outs = [False] * n, []
        for c, (roots, episodes, horizon) in enumerate(case["calls"]):
            reach = handle.info()["max_count"] + episodes * horizon
            rthr = gb.thresholds_by_count(gc.THRESHOLD, horizon, A, episodes, 1, reach)
            tthr = gb.thresholds_by_count(case["transition_threshold"], horizon, A, episodes, 1, reach)
            out = handle.plan(roots, episodes, horizon, gc.GAMMA, gc.VMAX, gc.ACCURACY, gc.TIMEOUT, rthr, tthr, rng)
            assert_form(ctx, gc.FORM[mode] + "_" + placement)
            RECORDED.add(ctx.last_kernel_variant())
            for i, p in enumerate(ref["planners"]):
                want, tag = p["calls"][c], (case["name"], c, i)
                failed[i] = failed[i] or (queue_cap is not None and want["peak"] > queue_cap)
                if failed[i]:
                    assert int(out["status"][i]) == native.MP_ERR_ALLOC and int(out["plan_len"][i]) == 0, tag
                    assert int(out["plans"].reshape(-1)[i]) == -1, tag
                    continue
                assert int(out["status"][i]) == native.MP_OK, tag
                assert device_plan(out, i, order) == want["plan"], tag
                assert np.array_equal(rng[i], want["rng_after"]), tag
                assert (int(out["env_steps"][i]), int(out["pops"][i])) == (want["steps"], want["pops"]), tag
                if want["listing"] is not None:
                    assert gb.compare_listing(listing_in_env_ids(handle.export(i), order), want["listing"], TOL) == [], tag
            outs.append(out)
        exports = [handle.export(i) for i in range(n)]
        return (outs, exports, failed)
    finally:
        handle.close()
        model.close()


@pytest.mark.parametrize("name", tuple(gc.WIDE))
def test_more_than_64_actions(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    assert not gc.set_aside(name) and case["reward"].shape[1] > 64
    run_case(ctx, monkeypatch, case, ref)


@pytest.mark.parametrize("name", gc.FAMILIES["ring"][0])
def test_more_than_64_states_in_one_episode(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    assert not gc.set_aside(name) and max(p["calls"][0]["uq"] for p in ref["planners"]) > 64
    run_case(ctx, monkeypatch, case, ref)


@pytest.mark.parametrize("name", gc.FAMILIES["hub"][0])
def test_more_than_64_parents(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    assert not gc.set_aside(name) and ref["planners"][0]["calls"][gc.HUB_LAST]["parents_before"][0] >= 65
    _, exports, _ = run_case(ctx, monkeypatch, case, ref)
    hub = int(np.nonzero(exports[0]["state"] == 0)[0][0])
    assert exports[0]["parent_ptr"][hub + 1] - exports[0]["parent_ptr"][hub] >= 65


@pytest.mark.parametrize("name", gc.FAMILIES["hub"][0])
def test_the_ring_wraps_at_a_capacity_the_pushes_exceed(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    cap, _ = gc.queue_caps(ref)
    last = [p["calls"][gc.HUB_LAST] for p in ref["planners"]]
    assert max(c["pushed"] for c in last) > cap >= max(c["peak"] for c in last)
    _, _, failed = run_case(ctx, monkeypatch, case, ref, queue_cap=cap)
    assert failed == [False, False, False]


@pytest.mark.parametrize("name", gc.FAMILIES["hub"][0])
def test_queue_overflow_is_reported_per_planner_and_stays(ctx, monkeypatch, refs, name):
    """Half the capacity: the planners whose restated peak exceeds it answer MP_ERR_ALLOC with an empty plan in the hub's own
    plan and again in the call after it; the third planner of the batch, whose hub has one parent, equals the restatement in
    both."""
    case, ref = refs[name]
    _, half = gc.queue_caps(ref)
    outs, _, failed = run_case(ctx, monkeypatch, case, ref, queue_cap=half)
    assert failed == [True, True, False]
    for out in outs[gc.HUB_LAST:]:
        assert out["status"].tolist() == [native.MP_ERR_ALLOC, native.MP_ERR_ALLOC, native.MP_OK]
    assert all((out["status"] == 0).all() for out in outs[:gc.HUB_LAST])


def test_an_update_queue_longer_than_the_ring_is_an_overflow_too(ctx, monkeypatch, refs):
    """`nq > qcap`: the episode's own update_queue does not fit the ring of 64, before any parent is appended."""
    case, ref = refs["tail_table"]
    assert [p["calls"][0]["uq"] > 64 for p in ref["planners"]] == [True, True, False]
    outs, _, failed = run_case(ctx, monkeypatch, case, ref, queue_cap=64)
    assert failed == [True, True, False]
    assert outs[0]["status"].tolist() == [native.MP_ERR_ALLOC, native.MP_ERR_ALLOC, native.MP_OK]


def test_queue_capacity_through_the_agent(refs):
    """planner.queue_capacity reaches mp_gbop_create; a full queue raises RuntimeError naming it, and the planner stays failed."""
    case, ref = refs["hub_table"]
    _, half = gc.queue_caps(ref)
    env = FiniteMDPEnv(dict(mode="deterministic", transition=case["transition"].tolist(), reward=case["reward"].tolist(),
                            terminal=[0] * gc.HUB_S, state=1, max_steps=0))
    env.reset()
    cfg = {"__class__": GBOP_AGENT, "gamma": gc.GAMMA, "accuracy": gc.ACCURACY, "max_next_states_count": 1, "episodes": 2,
           "horizon": 1,
           "upper_bound": {"type": "kullback-leibler", "threshold": gc.THRESHOLD, "transition_threshold": gc.TRANSITION_THRESHOLD}}
    agent = agent_factory(env, cfg)
    planner = agent.planner
    planner.queue_capacity = half
    agent.seed(3)
    for s in range(1, 71):                       # every root adds itself to the hub's parents (a table: each step leads there)
        env.mdp.state = s
        assert len(agent.plan(s)) == 2
    assert planner._device[2].info()["queue_cap"] == half
    planner.config.update(episodes=3, horizon=2)
    env.mdp.state = 0
    for _ in range(2):
        with pytest.raises(RuntimeError, match="queue_capacity, or MP_GBOP_QUEUE"):     # the knob mp_gbop_create reads
            agent.plan(0)


@pytest.mark.parametrize("name", tuple(gc.SMALL_FORMS))
def test_both_placements_give_the_same_bits_in_every_mode(ctx, monkeypatch, refs, name):
    both_placements(ctx, monkeypatch, refs, name)


def both_placements(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    assert not gc.set_aside(name)
    lds = run_case(ctx, monkeypatch, case, ref, placement="lds")
    monkeypatch.setenv("MP_GBOP_LDS_BYTES", "0")
    glob = run_case(ctx, monkeypatch, case, ref, placement="global")
    monkeypatch.delenv("MP_GBOP_LDS_BYTES")
    for x, y in zip(lds[0], glob[0]):
        for k in x:
            assert np.array_equal(x[k], y[k]), k            # the same arithmetic wherever the bounds live: by bits
    for x, y in zip(lds[1], glob[1]):
        assert gb.compare_listing(x, y, 0.0) == []


@pytest.mark.parametrize("name,placement",
                         [("limit_sparse_1024", "lds"), ("limit_sparse_1025", "global"), ("limit_table_1025", "global")])
def test_the_natural_lds_limit_without_a_knob(ctx, monkeypatch, refs, name, placement):
    monkeypatch.delenv("MP_GBOP_LDS_BYTES", raising=False)
    case, ref = refs[name]
    assert not gc.set_aside(name)
    run_case(ctx, monkeypatch, case, ref, placement=placement)


def test_every_form_name_was_recorded_in_this_file(ctx, monkeypatch, refs):
    """(Run on its own, the test launches the forms the file's other tests would have.)"""
    for name in gc.SMALL_FORMS:
        mode = refs[name][0]["mode"]
        if not {gc.FORM[mode] + "_lds", gc.FORM[mode] + "_global"} <= RECORDED:
            both_placements(ctx, monkeypatch, refs, name)
    assert RECORDED == set(native.gbop_form_names())
