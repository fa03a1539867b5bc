"""GBOP on the device (mp_gbop_*, rl_agents_amd/csrc/gbop.hip) against the reference's own outputs (tests/golden/gbop.npz)
and the test-side restatement (tests/gbop_restatement.py).

Parity: plans with their keys, statuses, env steps, generator records, creation order, parents in order, every count, every
placeholder assignment and reward sum exactly; bounds and p_plus / p_minus within 1e-12 / (1 - gamma) (the
device sums in the butterfly's order and uses its own log / exp)."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, generators
from tests import gbop_restatement as gb
from tests.helpers import assert_form
from tests.test_gbop_host import (BOUND_TOL, GBOP_AGENT, GOLDEN, case_config, case_env, generator_from, golden_case, golden_graph,
                                  golden_plan, names, thresholds_of)

pytestmark = pytest.mark.gpu

STATUS = {"ValueError/placeholders": native.ERR_GBOP_PLACEHOLDERS, "TypeError/default_config": native.ERR_GBOP_REWARD_THRESHOLD}
FORM = {"deterministic": "gbop_table", "stochastic": "gbop_dense", "sparse": "gbop_sparse"}
ZERO = {"type": "kullback-leibler", "threshold": "0*np.log(time)", "transition_threshold": "0.1*np.log(time)"}
MARGIN = 1e-9


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def load_model(ctx, mode, transition, reward, next_states=None, available=None):
    if mode == "deterministic":
        return ctx.load_table(transition, reward, None, available=available)
    model = ctx.load_dense(transition, reward, None) if mode == "stochastic" else ctx.load_sparse(transition, next_states, reward, None)
    if available is not None:
        model.set_available(available)
    return model


def tables(expr_r, expr_t, horizon, actions, episodes, reach):
    return (gb.thresholds_by_count(expr_r, horizon, actions, episodes, 1, max(reach, 1)),
            gb.thresholds_by_count(expr_t, horizon, actions, episodes, 1, max(reach, 1)))


def device_listing(handle, model, i=0):
    lst = handle.export(i)
    order = getattr(model, "action_order", None)
    if order is not None:
        act = lst["action"]
        lst["action"] = np.where(act >= 0, np.asarray(order)[np.maximum(act, 0)], -1).astype(np.int32)
    return lst


def device_plan(out, i, order=None):
    n = int(out["plan_len"][i])
    a = int(np.asarray(out["plans"]).reshape(-1)[i])
    plan = [a if order is None else int(order[a])] if n >= 1 else []
    if n >= 2:
        key = int(out["key"][i])
        plan.append("placeholder_{}".format(-1 - key) if key < 0 else str(key))
    return plan


def test_every_golden_case_through_the_c_abi(z):
    plans = 0
    for name in names(z):
        case = golden_case(z, name)
        if name == "no_listed_action":
            # a state without a listed action cannot reach the planner: the library refuses such an availability table when
            # it is loaded, so the kernel's MP_ERR_GBOPD_NO_ACTION stands behind a door that is shut
            c = native.Context(0)
            try:
                with pytest.raises(native.NativeError) as e:
                    load_model(c, str(case["mdp/mode"]), case["mdp/transition"], case["mdp/reward"], case.get("mdp/next"),
                               case["available"])
                assert e.value.code == native.MP_ERR_ARG
            finally:
                c.close()
            plans += int(case["n_plans"])
            continue
        plans += len(plan_golden_case(case, name)[1])
    assert plans == sum(int(z["gbop/{}/n_plans".format(n)]) for n in names(z))


def plan_golden_case(case, name, n_plans=None, placement="lds"):
    """Every plan of a golden case (or its first ``n_plans``) on one kept planner through the C ABI, each held to the golden:
    kernel form, status, generator record, plan, steps, the exported graph and the root's bounds.
    -> the handle's info and, per plan, (outputs, generator record, listing)."""
    env = case_env(case)
    planner = agent_factory(env, case_config(case)).planner
    model = planner.model_for(env)
    order = getattr(model, "action_order", None)
    K, gamma = int(case["max_next_states_count"]), float(case["gamma"])
    episodes, horizon, A = int(case["episodes"]), int(case["horizon"]), case["mdp/reward"].shape[1]
    handle = native.StochasticGraphBasedPlanners(planner.models.ctx, model, 1, K)
    tol = BOUND_TOL / (1 - gamma)
    steps, records = 0, []
    for i in range(int(case["n_plans"]) if n_plans is None else n_plans):
        reach = handle.info()["max_count"] + episodes * horizon
        rthr, tthr = tables(str(case["threshold"]), str(case["transition_threshold"]), horizon, A, episodes, reach)
        rng = case["plan{}/rng_before".format(i)].copy().reshape(1, 6)
        out = handle.plan([int(case["roots"][i])], episodes, horizon, gamma, 1 / (1 - gamma), float(case["accuracy"]),
                          int(case["sampling_timeout"]), rthr, tthr, rng)
        tag = (name, i)
        assert_form(planner.models.ctx, FORM[str(case["mdp/mode"])] + "_" + placement)
        assert planner.models.ctx.last_kernel_variant() in native.gbop_form_names()
        error = str(case["plan{}/error".format(i)])
        assert int(out["status"][0]) == (STATUS[error + "/" + name] if error else native.MP_OK), tag
        assert np.array_equal(rng[0], case["plan{}/rng_after".format(i)]), tag
        assert device_plan(out, 0, order) == golden_plan(case, i), tag
        steps += int(out["env_steps"][0])
        assert steps == int(case["plan{}/env_steps".format(i)]), tag
        ref = golden_graph(case, i)
        lst = device_listing(handle, model)
        assert gb.compare_listing(lst, ref, tol) == [], tag
        if not error:
            r = int(ref["root"])
            assert abs(out["value_lower"][0] - ref["lower"][r]) <= tol and abs(out["value_upper"][0] - ref["upper"][r]) <= tol, tag
        records.append((out, rng, lst))
    info = handle.info()
    handle.close()
    return info, records


def test_each_knob_moves_only_its_own_planner(z, monkeypatch):
    """The shared host helpers take the knob's name from their caller: GBOP-D's three leave a GBOP planner as it is -- the
    default ring, both bounds in LDS, and no pop limit of 1: the golden's statuses and the unknobbed run's bits -- and GBOP's
    own move it."""
    for knob in ("MP_GBOPD_QUEUE", "MP_GBOPD_LDS_BYTES", "MP_GBOPD_MAX_POPS", "MP_GBOP_QUEUE", "MP_GBOP_LDS_BYTES", "MP_GBOP_MAX_POPS"):
        monkeypatch.delenv(knob, raising=False)
    name = next(n for n in names(z) if n != "no_listed_action" and int(z["gbop/{}/n_plans".format(n)]) >= 2 and not any(
        str(z["gbop/{}/plan{}/error".format(n, i)]) for i in range(2)))
    case = golden_case(z, name)
    info, plain = plan_golden_case(case, name, 2)
    assert info["queue_cap"] == 65536
    assert all(int(out["status"][0]) == native.MP_OK for out, _, _ in plain)
    assert max(int(out["pops"][0]) for out, _, _ in plain) > 1           # (a pop limit of 1 would end these plans)
    monkeypatch.setenv("MP_GBOPD_QUEUE", "100")
    monkeypatch.setenv("MP_GBOPD_LDS_BYTES", "0")
    monkeypatch.setenv("MP_GBOPD_MAX_POPS", "1")
    info, other = plan_golden_case(case, name, 2)                       # (the LDS form is asserted for every plan in there)
    assert info["queue_cap"] == 65536
    for (out, rng, lst), (out_o, rng_o, lst_o) in zip(plain, other):
        assert all(out[k].tobytes() == out_o[k].tobytes() for k in out) and np.array_equal(rng, rng_o)
        assert gb.compare_listing(lst_o, lst, 0.0) == []
    monkeypatch.setenv("MP_GBOP_QUEUE", "100")
    assert plan_golden_case(case, name, 0)[0]["queue_cap"] == 128       # (a new batch: nothing is planned on the small ring)
    monkeypatch.delenv("MP_GBOP_QUEUE")
    monkeypatch.setenv("MP_GBOP_LDS_BYTES", "0")
    assert plan_golden_case(case, name, 2, placement="global")[0]["queue_cap"] == 65536


def test_every_golden_case_through_the_agent(z):
    from rl_agents_amd.gbop import build_graph
    for name in names(z):
        if name == "no_listed_action":
            continue                                     # (refused when the table is loaded: the test above asserts it)
        case = golden_case(z, name)
        env = case_env(case)
        agent = agent_factory(env, case_config(case))
        planner = agent.planner
        assert (int(planner.config["episodes"]), int(planner.config["horizon"])) == (int(case["episodes"]), int(case["horizon"])), name
        tol = BOUND_TOL / (1 - float(case["gamma"]))
        for i in range(int(case["n_plans"])):
            env.mdp.state = int(case["roots"][i])
            native.generator_set_state(planner.np_random, case["plan{}/rng_before".format(i)])
            error, tag = str(case["plan{}/error".format(i)]), (name, i)
            if error:
                with pytest.raises({"ValueError": ValueError, "TypeError": TypeError}[error]) as raised:
                    agent.plan(int(case["roots"][i]))
                assert str(raised.value) == str(case["plan{}/message".format(i)]), tag
            else:
                assert agent.plan(int(case["roots"][i])) == golden_plan(case, i) == planner.get_plan(), tag
            # the draws and steps made before the reference raised
            assert np.array_equal(native.rng_state_from_generator(planner.np_random), case["plan{}/rng_after".format(i)]), tag
            assert planner.env_steps == int(case["plan{}/env_steps".format(i)]), tag
            ref = golden_graph(case, i)
            assert gb.compare_listing(device_listing(planner._device[2], planner._device[0]), ref, tol) == [], tag
            nodes, want = planner.nodes, build_graph(ref)
            assert list(nodes) == list(want), tag
            for k in nodes:
                assert list(nodes[k].children) == list(want[k].children), tag
                assert [p.observation for p in nodes[k].parents] == [p.observation for p in want[k].parents], tag
                for a in nodes[k].children:
                    assert list(nodes[k].children[a].children) == list(want[k].children[a].children), tag
                    assert nodes[k].children[a].next_states == want[k].children[a].next_states, tag
            if not error:
                assert planner.root is nodes[str(int(case["roots"][i]))], tag
            visits = np.zeros(len(ref["visits"]), np.int64)
            for k, v in planner.get_visits().items():
                visits[int(k)] = v
            assert np.array_equal(visits, ref["visits"]), tag


# ---- the sweep: small random models, the smallest shapes at which the kernel can still go wrong
def sweep_model(seed, S, A, B):
    """A sparse model of B successors a row with a self-loop in every state's first action; rewards in [0, 1]."""
    rng = np.random.default_rng(1000 + seed)
    nxt = rng.integers(0, S, size=(S, A, B))
    nxt[:, 0, 0] = np.arange(S)
    P = rng.dirichlet(np.ones(B), size=(S, A))
    reward = np.round(rng.random((S, A)), 3)
    return P, nxt, reward


SWEEP = [  # seed, mode, S, A, B (successors a row), K, episodes, horizon
    (0, "sparse", 2, 1, 2, 2, 5, 3), (1, "sparse", 3, 2, 2, 3, 5, 4), (2, "dense", 5, 2, 2, 2, 6, 3), (3, "sparse", 17, 5, 2, 2, 6, 4),
    (4, "table", 5, 5, 1, 1, 5, 4), (5, "table", 17, 2, 1, 3, 5, 5), (6, "sparse", 5, 1, 2, 32, 5, 3), (7, "dense", 3, 5, 3, 32, 4, 4),
    (8, "sparse", 17, 2, 3, 3, 3, 70), (9, "sparse", 5, 2, 2, 2, 8, 1), (10, "sparse", 5, 2, 3, 2, 6, 4), (11, "dense", 17, 1, 2, 1, 6, 3),
    (12, "table", 2, 2, 1, 2, 6, 1), (13, "sparse", 3, 5, 2, 1, 4, 3), (14, "dense", 2, 5, 2, 3, 5, 66), (15, "sparse", 17, 5, 3, 32, 3, 5),
    (16, "table", 3, 1, 1, 32, 4, 3), (17, "sparse", 2, 2, 2, 1, 5, 2), (18, "dense", 5, 5, 2, 3, 4, 3), (19, "sparse", 3, 2, 3, 2, 5, 3),
]
N_PLANNERS = 5          # more planners than workgroups: the grid is lowered to 2


def sweep_reference(case):
    """The restatement's answer for every planner of a sweep case, each on its own root, with the smallest margin seen."""
    seed, mode, S, A, B, K, episodes, horizon = case
    P, nxt, reward = sweep_model(seed, S, A, B)
    if mode == "table":
        args = ("deterministic", nxt[:, :, 0], reward, 0.8, K, None)
    elif mode == "dense":
        dense = np.zeros((S, A, S))
        for s in range(S):
            for a in range(A):
                for b in range(B):
                    dense[s, a, nxt[s, a, b]] += P[s, a, b]
        args = ("stochastic", dense, reward, 0.8, K, None)
    else:
        args = ("sparse", P, reward, 0.8, K, nxt)
    rng = native.seed_sequence_states((), 500 + seed, N_PLANNERS)
    roots = [(seed + 3 * i) % S for i in range(N_PLANNERS)]
    zero, tthr = (lambda c: 0.0), (lambda c: gb.thresholds_by_count(ZERO["transition_threshold"], horizon, A, episodes, c, c)[0])
    results, pairs = [], []
    for i in range(N_PLANNERS):
        graph, gen = gb.Graph(*args), generator_from(rng[i])
        try:
            plan, error = graph.plan(roots[i], episodes, horizon, 1e-2, zero, tthr, gen,
                                     observe=lambda kind, a, b: pairs.append((float(a), float(b)))), None
        except ValueError as e:
            plan, error = [], e
        results.append((plan, error, native.rng_state_from_generator(gen), graph))
    return args, rng, roots, results, gb.smallest_margin(pairs)


@pytest.fixture(scope="module")
def sweep():
    return {case[0]: sweep_reference(case) for case in SWEEP}


def test_sweep_sets_aside_at_most_one_case_in_ten(sweep):
    fragile = [seed for seed, ref in sweep.items() if ref[4] <= MARGIN]
    assert len(fragile) * 10 <= len(SWEEP), fragile
    errors = [seed for seed, ref in sweep.items() if any(r[1] is not None for r in ref[3])]
    assert errors and len(errors) < len(SWEEP) // 2          # rows with more successors than K are among the cases
    assert {c[2] for c in SWEEP} == {2, 3, 5, 17} and {c[3] for c in SWEEP} == {1, 2, 5} and {c[5] for c in SWEEP} == {1, 2, 3, 32}
    assert any(c[7] == 1 for c in SWEEP) and any(c[7] > 64 for c in SWEEP) and any(c[4] > c[5] for c in SWEEP)


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "seed{}".format(c[0]))
def test_sweep_against_the_restatement(case, sweep, ctx, monkeypatch):
    seed, mode, S, A, B, K, episodes, horizon = case
    args, rng, roots, results, margin = sweep[seed]
    if margin <= MARGIN:
        return      # set aside as margin-fragile by the restatement: counted in test_sweep_sets_aside_at_most_one_case_in_ten
    monkeypatch.setenv("MP_GBOP_GRID", "2")
    model = load_model(ctx, args[0], args[1], args[2], args[5])
    handle = native.StochasticGraphBasedPlanners(ctx, model, N_PLANNERS, K)
    try:
        rthr, tthr = tables(ZERO["threshold"], ZERO["transition_threshold"], horizon, A, episodes, episodes * horizon)
        dev_rng = rng.copy()
        out = handle.plan(roots, episodes, horizon, 0.8, 1 / (1 - 0.8), 1e-2, 100, rthr, tthr, dev_rng)
        assert_form(ctx, {"table": "gbop_table", "dense": "gbop_dense", "sparse": "gbop_sparse"}[mode] + "_lds")
        for i, (plan, error, rng_after, graph) in enumerate(results):
            tag = (seed, i)
            assert int(out["status"][i]) == (native.MP_OK if error is None else native.ERR_GBOP_PLACEHOLDERS), tag
            assert device_plan(out, i) == plan, tag
            assert np.array_equal(dev_rng[i], rng_after), tag
            assert int(out["env_steps"][i]) == graph.n_observations and int(out["pops"][i]) == graph.pops, tag
            assert gb.compare_listing(handle.export(i), graph.listing(), BOUND_TOL / (1 - 0.8)) == [], tag
    finally:
        handle.close()
        model.close()


def test_a_self_loop_makes_a_node_its_own_parent(sweep):
    graph = sweep[0][3][0][3]
    lst = graph.listing()
    assert any(i in lst["parent_idx"][lst["parent_ptr"][i]:lst["parent_ptr"][i + 1]] for i in range(len(lst["state"])))


def kept_case():
    tab = generators.random_sparse(9, 3, 2, seed=31)
    cfg = {"__class__": GBOP_AGENT, "budget": 60, "gamma": 0.8, "upper_bound": ZERO, "max_next_states_count": 2}
    env = FiniteMDPEnv(dict(tab, state=0, max_steps=0))
    env.reset()
    return tab, cfg, env


def restated(tab, planner, roots):
    """The restatement's plans on ``roots`` in turn on ONE graph, from a copy of the planner's generator as it stands."""
    pc = planner.config
    graph = gb.Graph(str(tab["mode"]), tab["transition"], tab["reward"], pc["gamma"], pc["max_next_states_count"], tab.get("next"))
    gen = generator_from(native.rng_state_from_generator(planner.np_random))
    A = np.asarray(tab["reward"]).shape[1]
    tthr = lambda c: gb.thresholds_by_count(pc["upper_bound"]["transition_threshold"], pc["horizon"], A, pc["episodes"], c, c)[0]  # noqa: E731
    plans = [graph.plan(s, pc["episodes"], pc["horizon"], pc["accuracy"], lambda c: 0.0, tthr, gen) for s in roots]
    return plans, graph, gen


def test_kept_graph_three_plans_forget_and_changed_tables():
    tab, cfg, env = kept_case()
    agent = agent_factory(env, cfg)
    agent.seed(7)
    planner = agent.planner
    roots = [0, 4, 0]
    plans, graph, gen = restated(tab, planner, roots)
    tol = BOUND_TOL / (1 - 0.8)
    evaluations = []
    for s, plan in zip(roots, plans):
        env.mdp.state = s
        assert agent.plan(s) == plan
        evaluations.append(planner.tables.evaluations)
    assert np.array_equal(native.rng_state_from_generator(planner.np_random), native.rng_state_from_generator(gen))
    assert gb.compare_listing(planner._device[2].export(0), graph.listing(), tol) == []
    per_plan = int(planner.config["episodes"]) * int(planner.config["horizon"])
    assert evaluations == [per_plan, 2 * per_plan, 3 * per_plan]           # the tables grew by the new counts only
    assert planner._device[2].info()["max_count"] == 3 * per_plan
    assert int(graph.c_count.max()) > int(planner.config["episodes"])        # counts grew past one plan's
    agent.reset()                                                           # reset() replaces only the root: the graph is kept
    assert len(planner.nodes) == len(graph.created)
    # forget() starts over: the next plan is a fresh planner's
    planner.forget()
    assert planner.nodes == {}
    agent.seed(8)
    fresh_plans, fresh, _ = restated(tab, planner, [4])
    env.mdp.state = 4
    assert agent.plan(4) == fresh_plans[0]
    assert gb.compare_listing(planner._device[2].export(0), fresh.listing(), tol) == []
    # tables changed under the kept graph are refused, by the library and by the agent
    model, handle = planner._device[0], planner._device[2]
    model.set_available(generators.random_available(9, 3, seed=32, rate=0.4))
    with pytest.raises(native.NativeError, match="kept graph") as e:
        handle.export(0)
    assert e.value.code == native.MP_ERR_ARG
    with pytest.raises(NotImplementedError, match="previous tables"):
        agent.plan(4)


def test_both_placements_and_device_arrays_equal_host_arrays(ctx, monkeypatch):
    import torch
    tab = generators.random_sparse(12, 3, 2, seed=41)
    n, K, episodes, horizon, gamma = 4, 2, 8, 5, 0.8
    roots = np.asarray([0, 3, 7, 11], np.int32)
    rthr, tthr = tables(ZERO["threshold"], ZERO["transition_threshold"], horizon, 3, episodes, 2 * episodes * horizon + 1)
    model = load_model(ctx, "sparse", tab["transition"], tab["reward"], tab["next"])
    results = {}
    for placement, limit in (("lds", None), ("global", "0")):
        if limit is not None:
            monkeypatch.setenv("MP_GBOP_LDS_BYTES", limit)
        handle = native.StochasticGraphBasedPlanners(ctx, model, n, K)
        rng = native.seed_sequence_states((), 77, n)
        outs = []
        for _ in range(2):
            outs.append(handle.plan(roots, episodes, horizon, gamma, 1 / (1 - gamma), 1e-2, 100, rthr, tthr, rng))
            assert_form(ctx, "gbop_sparse_" + placement)
            assert (outs[-1]["status"] == 0).all()
        results[placement] = (outs, rng, [handle.export(i) for i in range(n)])
        handle.close()
    (a, rng_a, lst_a), (b, rng_b, lst_b) = results["lds"], results["global"]
    assert np.array_equal(rng_a, rng_b)
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k], y[k]), k                # the same arithmetic wherever the bounds live: by bits
    for x, y in zip(lst_a, lst_b):
        assert gb.compare_listing(x, y, 0.0) == []
    # MP_MEM_DEVICE: one asynchronous launch on device buffers gives what the host-array call gives
    monkeypatch.delenv("MP_GBOP_LDS_BYTES", raising=False)
    handle = native.StochasticGraphBasedPlanners(ctx, model, n, K)
    rng = native.seed_sequence_states((), 77, n)
    d_rng = torch.from_numpy(rng.view(np.int64).copy()).cuda()
    i32 = lambda fill=0: torch.full((n,), fill, dtype=torch.int32, device="cuda")  # noqa: E731
    d = dict(action=i32(), key=i32(), plan_len=i32(), value_lower=torch.zeros(n, dtype=torch.float64, device="cuda"),
             value_upper=torch.zeros(n, dtype=torch.float64, device="cuda"), env_steps=torch.zeros(n, dtype=torch.int64, device="cuda"),
             pops=torch.zeros(n, dtype=torch.int64, device="cuda"), status=i32(7))
    d_roots = torch.from_numpy(roots).cuda()
    for call in range(2):
        torch.cuda.synchronize()
        handle.plan_device(d_roots, episodes, horizon, gamma, 1 / (1 - gamma), 1e-2, 100, rthr, tthr, d_rng, **d)
        ctx.synchronize()
        for k, name in (("plans", "action"), ("key", "key"), ("plan_len", "plan_len"), ("value_lower", "value_lower"),
                        ("value_upper", "value_upper"), ("env_steps", "env_steps"), ("pops", "pops"), ("status", "status")):
            assert np.array_equal(d[name].cpu().numpy(), a[call][k]), (call, k)
    assert np.array_equal(d_rng.cpu().numpy().view(np.uint64), rng_a)
    for i in range(n):
        assert gb.compare_listing(handle.export(i), lst_a[i], 0.0) == []
    # a root out of range in a device array: that planner answers MP_ERR_ARG, the others plan
    torch.cuda.synchronize()
    handle.plan_device(torch.tensor([0, 12, -1, 3], dtype=torch.int32, device="cuda"), 1, 1, gamma, 1 / (1 - gamma), 1e-2, 100,
                       rthr, tthr, d_rng, **d)
    ctx.synchronize()
    assert d["status"].cpu().numpy().tolist() == [0, native.MP_ERR_ARG, native.MP_ERR_ARG, 0]
    handle.close()
    model.close()


def test_refused_arguments_and_models(ctx):
    det = generators.random_deterministic(10, 3, seed=3)
    model = ctx.load_table(det["transition"], det["reward"], det["terminal"])
    for K in (0, 33, -1):
        with pytest.raises(native.NativeError) as e:
            native.StochasticGraphBasedPlanners(ctx, model, 1, K)
        assert e.value.code == native.MP_ERR_ARG
    handle = native.StochasticGraphBasedPlanners(ctx, model, 1, 2)
    rng = native.seed_sequence_states((), 1, 1)
    short = np.zeros(5)
    with pytest.raises(native.NativeError, match="threshold tables hold 5 counts") as e:        # tables must cover the counts
        handle.plan([0], 3, 4, 0.8, 5.0, 1e-2, 100, short, short, rng)
    assert e.value.code == native.MP_ERR_ARG
    handle.K = 3                                                                                # not the handle's K
    with pytest.raises(native.NativeError, match="chance records hold 2 children"):
        handle.plan([0], 1, 1, 0.8, 5.0, 1e-2, 100, short, short, rng)
    handle.K = 2
    handle.close()
    for bad in (ctx.load_joint(np.stack([det["transition"]] * 2), np.stack([det["reward"]] * 2)),
                ctx.load_table_batch(np.stack([det["transition"]] * 2), np.stack([det["reward"]] * 2))):
        with pytest.raises(native.NativeError) as e:
            native.StochasticGraphBasedPlanners(ctx, bad, 1, 2)
        assert e.value.code == native.MP_ERR_MODE
        bad.close()
    model.close()


def test_one_certain_next_state_has_the_closed_form(ctx):
    """K = 1 on a deterministic table: every transition child is certain, so p_plus = p_minus = [1] and a chance node's
    bounds are mean + gamma * V of its next state, to the bit."""
    tab = generators.random_deterministic(8, 3, seed=51)
    gamma, episodes, horizon = 0.8, 10, 4
    model = ctx.load_table(tab["transition"], tab["reward"], None)
    handle = native.StochasticGraphBasedPlanners(ctx, model, 1, 1)
    rthr, tthr = tables(ZERO["threshold"], ZERO["transition_threshold"], horizon, 3, episodes, episodes * horizon)
    out = handle.plan([2], episodes, horizon, gamma, 1 / (1 - gamma), 1e-2, 100, rthr, tthr, native.seed_sequence_states((), 5, 1))
    assert out["status"][0] == 0 and out["plan_len"][0] == 2
    lst = handle.export(0)
    index = {int(s): i for i, s in enumerate(lst["state"])}
    checked = 0
    for i in range(len(lst["state"])):
        for k in range(int(lst["n_children"][i])):
            if lst["c_count"][i, k] == 0:
                continue
            s, a = int(lst["state"][i]), int(lst["action"][i, k])
            nxt = int(lst["k_state"][i, k, 0])
            assert nxt == int(tab["transition"][s][a]) and lst["k_count"][i, k, 0] == lst["c_count"][i, k]
            mean = lst["k_cum"][i, k, 0] / lst["k_count"][i, k, 0]
            assert lst["k_mu_ucb"][i, k, 0] == lst["k_mu_lcb"][i, k, 0] == mean
            assert lst["p_plus"][i, k].tolist() == [1.0] and lst["p_minus"][i, k].tolist() == [1.0]
            # (a bound is the value its last backup saw: it equals the closed form where the next state's bound has not moved since)
            assert lst["c_upper"][i, k] >= mean + gamma * lst["upper"][index[nxt]] - 1e-12
            assert lst["c_lower"][i, k] <= mean + gamma * lst["lower"][index[nxt]] + 1e-12
            checked += 1
    assert checked >= 3
    # the root's chance children were backed up by get_plan after the last pop: to the bit
    r = int(lst["root"])
    for k in range(int(lst["n_children"][r])):
        if lst["c_count"][r, k]:
            nxt = index[int(lst["k_state"][r, k, 0])]
            assert lst["c_lower"][r, k] == lst["k_mu_ucb"][r, k, 0] + gamma * lst["lower"][nxt]
    assert int(out["key"][0]) == int(tab["transition"][2][int(out["plans"][0])])
    handle.close()
    model.close()


def dense_env_config(seed):
    tab = dict(generators.random_sparse(8, 3, 2, seed=seed))
    dense = np.zeros((8, 3, 8))
    for s in range(8):
        for a in range(3):
            for b in range(2):
                dense[s, a, tab["next"][s][a][b]] += tab["transition"][s][a][b]
    return dict(mode="stochastic", transition=dense.tolist(), reward=tab["reward"], terminal=tab["terminal"], state=1, max_steps=4)


def test_a_plan_that_does_not_converge_is_ended_and_the_planner_stays_failed(monkeypatch):
    """The reference's partial value iteration need not end: max_expectation_under_constraint stops its Newton iteration at a
    step below 1e-2, so a chance node's bound is no monotone function of its children's, and bounds can move up and down by
    more than ``accuracy`` for ever (on this model the restatement's lower bounds of states 3 and 5 do, from the second plan of
    the episode on: 60 000 pops with the queue never empty).  The device ends such a plan at its pop limit (2^22, lowered here)
    with MP_ERR_GBOPD_DIVERGED, and the planner stays failed."""
    monkeypatch.setenv("MP_GBOP_MAX_POPS", "4000")
    env = FiniteMDPEnv(dense_env_config(61))
    env.reset()
    agent = agent_factory(env, {"__class__": GBOP_AGENT, "budget": 40, "gamma": 0.8, "upper_bound": ZERO, "max_next_states_count": 2})
    agent.seed(41)
    assert agent.plan(1) == [2, "7"]
    env.mdp.state = 7
    for _ in range(2):
        with pytest.raises(RuntimeError, match="queue pops without converging"):
            agent.plan(7)
    assert int(agent.planner._device[2].plan([7], 0, 1, 0.8, 5.0, 1e-2, 100, np.zeros(400), np.zeros(400),
                                             native.seed_sequence_states((), 1, 1))["status"][0]) == native.MP_ERR_GBOPD_DIVERGED


def test_host_stepped_batched_evaluation_equals_sequential_agents():
    """(accuracy 5e-2, that of the reference's planners_evaluation config: at 1e-2 the reference itself does not return from
    some plans on models of this kind -- see the test above.)"""
    from rl_agents_amd.trainer.batched_evaluation import BatchedEvaluation
    env_cfg = dense_env_config(64)
    cfg = {"__class__": GBOP_AGENT, "budget": 40, "gamma": 0.8, "accuracy": 5e-2, "upper_bound": ZERO, "max_next_states_count": 2}
    env = FiniteMDPEnv(env_cfg)
    env.reset()
    agent = agent_factory(env, cfg)
    n = 8
    out = BatchedEvaluation(env, agent, num_episodes=n, sim_seed=40, env_seed=9, device_resident="auto").run()
    assert out["device_resident"] is False
    for i in range(n):
        e = FiniteMDPEnv(env_cfg)
        e.reset()
        e.np_random = np.random.Generator(np.random.PCG64(np.random.SeedSequence([9, i])))
        seq = agent_factory(e, cfg)
        seq.seed(40 + i)
        actions, done = [], False
        while not done:
            a = seq.act(e.mdp.state)
            _, _, term, trunc, _ = e.step(a)
            actions.append(a)
            done = term or trunc
        assert out["lengths"][i] == len(actions), i
        np.testing.assert_array_equal(out["actions"][i, :len(actions)], actions)
