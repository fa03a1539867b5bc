"""GBOP-D on the device (mp_gbopd_*, rl_agents_amd/csrc/gbopd.hip) against the reference's own outputs
(tests/golden/gbopd.npz) and the test-side restatement (tests/gbopd_restatement.py).

Parity: everything exactly -- plans, both bounds of every node by their bits, creation order, children, rewards, parents in
order, the lifetime visit / update counters, len(observations) and the generator records, after EVERY plan."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv, generators
from tests import gbopd_restatement as gr
from tests.test_gbopd_host import GBOPD_AGENT, GOLDEN, generator_from, golden_case, golden_graph, graph_of, names

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def env_of(tab, s0=0, available=None, order=None):
    cfg = dict(mode="deterministic", transition=np.asarray(tab["transition"]).tolist(), reward=np.asarray(tab["reward"]).tolist(),
               terminal=np.asarray(tab["terminal"]).astype(int).tolist(), state=int(s0), max_steps=0)
    if order is not None:
        env = OrderedMaskedFiniteMDPEnv(dict(cfg, available=np.asarray(available).astype(int).tolist(),
                                             listing_order=[int(a) for a in order]))
    elif available is not None:
        env = MaskedFiniteMDPEnv(dict(cfg, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(cfg)
    env.reset()
    return env


def golden_env(case):
    tab = dict(transition=case["mdp/transition"], reward=case["mdp/reward"], terminal=case["mdp/terminal"])
    return env_of(tab, 0, case["available"] if bool(case["masked"]) else None, case["order"] if bool(case["ordered"]) else None)


def golden_config(case):
    return {"__class__": GBOPD_AGENT, "budget": int(case["budget"]), "gamma": float(case["gamma"]),
            "accuracy": float(case["accuracy"]), "sampling_timeout": int(case["sampling_timeout"]),
            "step_strategy": str(case["step_strategy"])}


def device_listing(planners, model, i=0):
    """mp_gbopd_export in the goldens' fields: action slots mapped back through the model's listing order."""
    lst = planners.export(i)
    order = getattr(model, "action_order", None)
    if order is not None:
        act = lst["child_action"]
        lst["child_action"] = np.where(act >= 0, np.asarray(order)[np.maximum(act, 0)], -1).astype(np.int32)
    return lst


def object_listing(planner):
    """The listing again from the planner's exported OBJECTS (planner.nodes, root, get_updates, get_visits)."""
    nodes = list(planner.nodes.values())
    index = {id(n): i for i, n in enumerate(nodes)}
    S, A = planner._device[0].S, planner._device[0].A
    n = len(nodes)
    out = dict(state=np.asarray([x.observation for x in nodes], np.int32), lower=np.asarray([x.value_lower for x in nodes]),
               upper=np.asarray([x.value_upper for x in nodes]), expanded=np.asarray([bool(x.children) for x in nodes], np.uint8),
               n_children=np.asarray([len(x.children) for x in nodes], np.int32), child_action=np.full((n, A), -1, np.int32),
               child_node=np.full((n, A), -1, np.int32), child_reward=np.zeros((n, A)))
    ptr, idx = [0], []
    for i, node in enumerate(nodes):
        for k, (a, child) in enumerate(node.children.items()):
            out["child_action"][i, k], out["child_node"][i, k], out["child_reward"][i, k] = a, index[id(child)], node.rewards[a]
        idx.extend(index[id(p)] for p in node.parents)
        ptr.append(len(idx))
    out["parent_ptr"], out["parent_idx"] = np.asarray(ptr, np.int32), np.asarray(idx, np.int32)
    for key, counts in (("updates", planner.get_updates()), ("visits", planner.get_visits())):
        out[key] = np.zeros(S, np.int64)
        for k, v in counts.items():
            out[key][int(k)] = v
    out["n_observations"] = np.asarray(planner.env_steps)
    out["root"] = np.asarray(index[id(planner.root)] if planner.root is not None else -1)
    return out


def plan_golden_case(case, name, n_plans=None):
    """Every plan of a golden case (or its first ``n_plans``) on one kept planner through the C ABI, each held to the golden:
    status, generator record, plan, the exported graph by bits, the root's bounds, len(observations).
    -> the handle's info and, per plan, (outputs, generator record, listing, kernel form)."""
    env = golden_env(case)
    planner = agent_factory(env, golden_config(case)).planner
    model = planner.model_for(env)
    order = getattr(model, "action_order", None)
    handle = native.GraphBasedPlanners(planner.models.ctx, model, 1)
    gamma = float(case["gamma"])
    observations, records = 0, []
    for i in range(int(case["n_plans"]) if n_plans is None else n_plans):
        rng = case["plan{}/rng_before".format(i)].copy().reshape(1, 6)
        out = handle.plan([int(case["roots"][i])], int(case["budget"]), gamma, 1 / (1 - gamma), float(case["accuracy"]),
                          int(case["sampling_timeout"]), rng)
        form = planner.models.ctx.last_kernel_variant()
        tag = (name, i)
        assert out["status"][0] == 0, tag
        assert np.array_equal(rng[0], case["plan{}/rng_after".format(i)]), tag
        plan = out["plans"][0, :out["plan_len"][0]]
        plan = plan if order is None else np.asarray(order)[plan]
        assert plan.tolist() == case["plan{}/plan".format(i)].tolist(), tag
        assert (out["plans"][0, out["plan_len"][0]:] == -1).all(), tag
        ref = golden_graph(case, i)
        lst = device_listing(handle, model)
        assert gr.same_listing(lst, ref) == [], tag
        r = int(ref["root"])
        assert np.array_equal(out["value_lower"], ref["lower"][r:r + 1]) and np.array_equal(out["value_upper"], ref["upper"][r:r + 1]), tag
        observations += int(out["env_steps"][0])
        assert observations == int(ref["n_observations"]), tag
        records.append((out, rng, lst, form))
    info = handle.info()
    assert info["n_planners"] == 1
    handle.close()
    return info, records


def cases_that_construct(z):
    return [(name, case) for name, case in ((n, golden_case(z, n)) for n in names(z)) if not str(case["construct_error"])]


def test_every_golden_case_through_the_c_abi(z):
    plans = sum(len(plan_golden_case(case, name)[1]) for name, case in cases_that_construct(z))
    assert plans >= 60


def test_both_placements_of_every_golden_case_by_bits(z, monkeypatch):
    """Every golden case over all its plans on the kept graph with both bounds in LDS and, by MP_GBOPD_LDS_BYTES=0, in global
    memory: each is held to the golden inside plan_golden_case, and to the other here -- every output, the generator records and
    the export."""
    monkeypatch.delenv("MP_GBOPD_LDS_BYTES", raising=False)
    for name, case in cases_that_construct(z):
        _, lds = plan_golden_case(case, name)
        monkeypatch.setenv("MP_GBOPD_LDS_BYTES", "0")
        _, glob = plan_golden_case(case, name)
        monkeypatch.delenv("MP_GBOPD_LDS_BYTES")
        assert len(lds) == len(glob) == int(case["n_plans"])
        for i, ((out, rng, lst, form), (out_g, rng_g, lst_g, form_g)) in enumerate(zip(lds, glob)):
            assert (form, form_g) == ("gbopd_wave_lds", "gbopd_wave_global"), (name, i)
            assert sorted(out) == sorted(out_g)
            for k in out:
                assert out[k].dtype == out_g[k].dtype and out[k].tobytes() == out_g[k].tobytes(), (name, i, k)
            assert np.array_equal(rng, rng_g), (name, i)
            assert gr.same_listing(lst_g, lst) == [], (name, i)


def test_each_knob_moves_only_its_own_planner(z, monkeypatch):
    """The shared host helpers take the knob's name from their caller: GBOP's three leave a GBOP-D planner as it is -- the
    default ring, both bounds in LDS, and no pop limit of 1: status 0 and the golden's bits -- and GBOP-D's own move it."""
    for knob in ("MP_GBOPD_QUEUE", "MP_GBOPD_LDS_BYTES", "MP_GBOPD_MAX_POPS", "MP_GBOP_QUEUE", "MP_GBOP_LDS_BYTES", "MP_GBOP_MAX_POPS"):
        monkeypatch.delenv(knob, raising=False)
    name, case = next((n, c) for n, c in cases_that_construct(z) if int(c["n_plans"]) >= 2)
    info, plain = plan_golden_case(case, name, 2)
    assert info["queue_cap"] == 65536 and [r[3] for r in plain] == ["gbopd_wave_lds"] * 2
    assert max(int(r[0]["updates"][0]) for r in plain) > 1              # (a pop limit of 1 would end these plans)
    monkeypatch.setenv("MP_GBOP_QUEUE", "100")
    monkeypatch.setenv("MP_GBOP_LDS_BYTES", "0")
    monkeypatch.setenv("MP_GBOP_MAX_POPS", "1")
    info, other = plan_golden_case(case, name, 2)
    assert info["queue_cap"] == 65536 and [r[3] for r in other] == ["gbopd_wave_lds"] * 2
    for (out, rng, lst, _), (out_o, rng_o, lst_o, _) in zip(plain, other):
        assert all(out[k].tobytes() == out_o[k].tobytes() for k in out) and np.array_equal(rng, rng_o)
        assert gr.same_listing(lst_o, lst) == []
    monkeypatch.setenv("MP_GBOPD_QUEUE", "100")
    assert plan_golden_case(case, name, 0)[0]["queue_cap"] == 128       # (a new batch; its ring is too small to plan this case on)
    monkeypatch.delenv("MP_GBOPD_QUEUE")
    monkeypatch.setenv("MP_GBOPD_LDS_BYTES", "0")
    info, own = plan_golden_case(case, name, 2)
    assert info["queue_cap"] == 65536 and [r[3] for r in own] == ["gbopd_wave_global"] * 2


@pytest.mark.parametrize("S,form", [(1024, "gbopd_wave_lds"), (1025, "gbopd_wave_global")])
def test_the_natural_lds_limit_without_a_knob(S, form, monkeypatch):
    """16 * S bytes against the 16 KiB limit with no knob set: the last size whose bounds live in LDS and the first whose do
    not, both against the restatement."""
    monkeypatch.delenv("MP_GBOPD_LDS_BYTES", raising=False)
    tab = generators.random_deterministic(S, 3, seed=76)
    cfg = dict(budget=90, gamma=0.9, accuracy=1e-3, sampling_timeout=20)
    roots = [np.asarray([0, S - 1], np.int32), np.asarray([S - 1, 7], np.int32)]
    planner, _ = check_against_restatement(tab, None, None, cfg, roots)
    assert planner.models.ctx.last_kernel_variant() == form


def test_every_golden_case_and_the_episodes_through_the_agent(z):
    plans = 0
    for name in names(z):
        case = golden_case(z, name)
        env = golden_env(case)
        if str(case["construct_error"]):
            with pytest.raises(ZeroDivisionError):
                agent_factory(env, {"__class__": GBOPD_AGENT, "gamma": int(case["gamma"])})
            continue
        agent = agent_factory(env, golden_config(case))
        agent.seed(int(case["seed"]))
        planner = agent.planner
        for i in range(int(case["n_plans"])):
            tag = (name, i)
            if bool(case["reset_before"][i]):
                agent.reset()
            s = int(case["roots"][i])
            env.mdp.state = s
            assert np.array_equal(native.rng_state_from_generator(planner.np_random), case["plan{}/rng_before".format(i)]), tag
            expected = case["plan{}/plan".format(i)].tolist()
            if str(case["plan{}/error".format(i)]):
                with pytest.raises(IndexError):
                    agent.act(s)
            elif bool(case["via_act"][i]):
                assert agent.act(s) == expected[0], tag
                assert list(agent.previous_actions) == expected, tag
            else:
                assert agent.plan(s) == expected, tag
            assert np.array_equal(native.rng_state_from_generator(planner.np_random), case["plan{}/rng_after".format(i)]), tag
            assert gr.same_listing(object_listing(planner), golden_graph(case, i)) == [], tag
            plans += 1
    assert plans >= 60


def random_case(rng, case):
    wide = case % 8 == 7
    S, A = int(rng.integers(2, 60)), int(rng.integers(65, 90)) if wide else int(rng.integers(1, 10))
    tab = generators.random_deterministic(S, A, seed=5000 + case, terminal_rate=float(rng.choice([0.0, 0.2])))
    kind = int(rng.integers(0, 4))
    if kind == 1:
        tab["reward"] = np.round(np.asarray(tab["reward"]) * 2) / 2              # ties
    elif kind == 2:
        tab["reward"] = np.asarray(tab["reward"]) * 4.0 - 1.5                    # outside [0, 1]
    available = order = None
    if case % 3 == 1:
        available = generators.random_available(S, A, seed=6000 + case, rate=0.4)
        if case % 2:
            order = rng.permutation(A)
    cfg = dict(gamma=float(rng.choice([0.5, 0.8, 0.9, 0.95, 0.99])), accuracy=float(rng.choice([0.0, 1e-4, 1e-2, 0.3])),
               sampling_timeout=int(rng.choice([1, 3, 10, 100])), budget=int(rng.integers(0, 40 * A if not wide else 12 * A)))
    if cfg["accuracy"] == 0.0:
        # accuracy 0 runs to the exact fixed point.  The bounds move monotonically -- so the iteration ends, in the reference
        # as here -- only while 0 <= V <= 1 / (1 - gamma) holds for the initial bounds: rewards in [0, 1]
        cfg["gamma"] = min(cfg["gamma"], 0.8)
        if kind == 2:
            tab["reward"] = np.clip((np.asarray(tab["reward"]) + 1.5) / 4.0, 0.0, 1.0)
    return tab, available, order, cfg


def check_against_restatement(tab, available, order, cfg, roots_per_plan, queue_cap=None, sample=None):
    """A batch planned ``len(roots_per_plan)`` times in a row against one restated Graph per sampled planner."""
    env = env_of(tab, 0, available, order)
    planner = agent_factory(env, dict(cfg, __class__=GBOPD_AGENT)).planner
    planner.queue_capacity = queue_cap
    n = len(roots_per_plan[0])
    sample = range(n) if sample is None else sample
    graphs = {i: gr.Graph(tab["transition"], tab["reward"], planner.config["gamma"], available, order) for i in sample}
    rng = planner.batch_rng_states(n)
    outs = []
    for roots in roots_per_plan:
        rng0 = rng.copy()
        out = planner.plan_batch(env, roots, rng_states=rng)
        assert (out["status"] == 0).all()
        model = planner._device[0]
        for i in sample:
            gen = generator_from(rng0[i])
            g = graphs[i]
            before = g.n_observations, g.pops
            pc = planner.config
            plan = g.plan(int(roots[i]), pc["budget"], pc["accuracy"], pc["sampling_timeout"], gen)
            assert out["plans"][i, :out["plan_len"][i]].tolist() == plan, i
            assert np.array_equal(rng[i], native.rng_state_from_generator(gen)), i
            assert (int(out["env_steps"][i]), int(out["updates"][i])) == (g.n_observations - before[0], g.pops - before[1]), i
            assert gr.same_listing(device_listing(planner._device[2], model, i), g.listing()) == [], i
        outs.append({k: np.copy(v) for k, v in out.items()})
    return planner, outs


def test_fuzz_against_the_restatement():
    rng = np.random.default_rng(9731)
    for case in range(48):
        tab, available, order, cfg = random_case(rng, case)
        S = np.asarray(tab["reward"]).shape[0]
        n = int(rng.integers(1, 4))
        roots = [rng.integers(0, S, size=n).astype(np.int32) for _ in range(2)]
        check_against_restatement(tab, available, order, cfg, roots)


@pytest.mark.parametrize("n", [1, 64, 4096, 65536])
def test_batches_and_their_replay_one_at_a_time(n):
    tab = generators.random_deterministic(24, 3, seed=71, terminal_rate=0.1)
    cfg = dict(budget=60, gamma=0.9, accuracy=1e-2, sampling_timeout=20)
    roots = [((np.arange(n) * 7 + k) % 24).astype(np.int32) for k in (0, 5)]    # two consecutive plan_batch calls
    sample = sorted(set(np.linspace(0, n - 1, 64).astype(int).tolist()))
    planner, outs = check_against_restatement(tab, None, None, cfg, roots, queue_cap=1024, sample=sample[:8])
    assert planner._device[2].info()["queue_cap"] == 1024
    # a sample of 64 replayed one at a time: planners of their own, the same generator records
    env = env_of(tab)
    rng_all = planner.batch_rng_states(n)
    for i in sample:
        single = agent_factory(env, dict(cfg, __class__=GBOPD_AGENT)).planner
        rng = rng_all[i:i + 1].copy()
        for k, out in enumerate(outs):
            one = single.plan_batch(env, roots[k][i:i + 1], rng_states=rng)
            for key in ("plans", "plan_len", "value_lower", "value_upper", "env_steps", "updates", "status"):
                assert np.array_equal(one[key][0], out[key][i]), (i, k, key)
            assert np.array_equal(rng[0], out["rng_states"][i]), (i, k)
        assert gr.same_listing(single._device[2].export(0), planner._device[2].export(i)) == [], i
        single.forget()
    planner.forget()


def test_ten_thousand_states_from_global_memory():
    tab = generators.random_deterministic(10000, 4, seed=72)
    cfg = dict(budget=200, gamma=0.9, accuracy=1e-3, sampling_timeout=100)
    roots = [np.asarray([0, 17, 9999], np.int32), np.asarray([5, 17, 1234], np.int32)]
    planner, _ = check_against_restatement(tab, None, None, cfg, roots)
    assert planner.models.ctx.last_kernel_variant() == "gbopd_wave_global"
    small, _ = check_against_restatement(generators.random_deterministic(100, 4, seed=73), None, None, cfg,
                                         [np.asarray([0, 1], np.int32)])
    assert small.models.ctx.last_kernel_variant() == "gbopd_wave_lds"


def test_more_than_64_actions_with_ties_in_every_chunk():
    tab = generators.random_deterministic(20, 150, seed=74)
    tab["reward"] = np.zeros_like(np.asarray(tab["reward"]))                    # 150 exact ties: the chunked tie draw
    cfg = dict(budget=1500, gamma=0.8, accuracy=1e-2, sampling_timeout=100)
    check_against_restatement(tab, None, None, cfg, [np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32)])
    avail = generators.random_available(20, 150, seed=75, rate=0.5)
    check_against_restatement(tab, avail, np.random.default_rng(1).permutation(150), cfg, [np.arange(3, dtype=np.int32)])


def test_host_stepped_batched_evaluation_equals_sequential_agents():
    from rl_agents_amd.trainer.batched_evaluation import BatchedEvaluation
    tab = dict(generators.highway_shaped(3, 4, 10, seed=3))
    cfg = dict(__class__=GBOPD_AGENT, budget=100, gamma=0.85)
    for strategy in ("reset", "subtree"):
        env_cfg = dict(tab, state=2, max_steps=9)
        env = FiniteMDPEnv(env_cfg)
        env.reset()
        agent = agent_factory(env, dict(cfg, step_strategy=strategy))
        n = 6
        out = BatchedEvaluation(env, agent, num_episodes=n, sim_seed=40, device_resident="auto").run()
        assert out["device_resident"] is False
        for i in range(n):
            e = FiniteMDPEnv(env_cfg)
            e.reset()
            seq = agent_factory(e, dict(cfg, step_strategy=strategy))
            seq.seed(40 + i)
            actions, total, done = [], 0.0, False
            while not done:
                a = seq.act(e.mdp.state)
                _, r, term, trunc, _ = e.step(a)
                actions.append(a)
                total += r
                done = term or trunc
            assert out["lengths"][i] == len(actions)
            np.testing.assert_array_equal(out["actions"][i, :len(actions)], actions)
            assert out["returns"][i] == pytest.approx(total, abs=1e-12)


def test_device_array_form():
    import torch
    tab = generators.random_deterministic(40, 4, seed=76, terminal_rate=0.1)
    ctx = native.Context(0)
    try:
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        n, t, gamma = 5, 12, 0.9
        handle = native.GraphBasedPlanners(ctx, model, n, queue_cap=2048)
        rng = native.seed_sequence_states((), 3, n)
        graphs = [gr.Graph(tab["transition"], tab["reward"], gamma) for _ in range(n)]
        gens = [generator_from(rng[i]) for i in range(n)]
        d_rng = torch.from_numpy(rng.view(np.int64).copy()).cuda()
        d = dict(plans=torch.zeros((n, t), dtype=torch.int32, device="cuda"), plan_len=torch.zeros(n, dtype=torch.int32, device="cuda"),
                 value_lower=torch.zeros(n, dtype=torch.float64, device="cuda"), value_upper=torch.zeros(n, dtype=torch.float64, device="cuda"),
                 env_steps=torch.zeros(n, dtype=torch.int64, device="cuda"), updates=torch.zeros(n, dtype=torch.int64, device="cuda"),
                 status=torch.full((n,), 7, dtype=torch.int32, device="cuda"))
        for roots in ([0, 1, 2, 3, 39], [4, 1, 7, 3, 0]):
            d_roots = torch.tensor(roots, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            handle.plan_device(d_roots, 120, gamma, 1 / (1 - gamma), 1e-3, t, d_rng, **d)
            ctx.synchronize()
            assert (d["status"].cpu().numpy() == 0).all()
            for i in range(n):
                plan = graphs[i].plan(roots[i], 120, 1e-3, t, gens[i])
                assert d["plans"][i].cpu().numpy()[:int(d["plan_len"][i])].tolist() == plan, i
                assert np.array_equal(d_rng[i].cpu().numpy().view(np.uint64), native.rng_state_from_generator(gens[i])), i
                assert gr.same_listing(handle.export(i), graphs[i].listing()) == [], i
        # a root out of range in a device array: that planner answers MP_ERR_ARG, nothing is read or written for it
        d_roots = torch.tensor([0, 40, -1, 3, 2], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        handle.plan_device(d_roots, 8, gamma, 1 / (1 - gamma), 1e-3, t, d_rng, **d)
        ctx.synchronize()
        assert d["status"].cpu().numpy().tolist() == [0, native.MP_ERR_ARG, native.MP_ERR_ARG, 0, 0]
        handle.close()
        model.close()
    finally:
        ctx.close()


def test_queue_overflow_is_reported_per_planner_and_stays(z):
    """The library's error path for a backup queue that fills up: MP_ERR_ALLOC for that planner, now and in the next call;
    the other planners of the batch equal the restatement; the agent raises RuntimeError naming the capacity setting.
    Which planner overflows follows from the restatement's own queue peak: the ring holds ``queue_cap`` entries."""
    case = golden_case(z, "gamma099_acc1e4")
    tab = dict(transition=case["mdp/transition"], reward=case["mdp/reward"], terminal=case["mdp/terminal"])
    gamma, acc, t, budget = float(case["gamma"]), float(case["accuracy"]), int(case["sampling_timeout"]), int(case["budget"])
    assert (gamma, acc) == (0.99, 1e-4)
    cap, roots = 64, np.asarray([0, 8, 5], np.int32)             # root 8 queues thousands of entries, roots 0 and 5 a few dozen
    ctx = native.Context(0)
    try:
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        handle = native.GraphBasedPlanners(ctx, model, 3, queue_cap=cap)
        assert handle.info()["queue_cap"] == cap
        rng = np.stack([case["plan0/rng_before"]] * 3).copy()
        graphs = [graph_of(case) for _ in range(3)]
        gens = [generator_from(rng[i]) for i in range(3)]
        failed = [False] * 3
        for call, b in enumerate((budget, 8, 8)):
            out = handle.plan(roots, b, gamma, 1 / (1 - gamma), acc, t, rng)
            for i in range(3):
                if not failed[i]:
                    graphs[i].queue_peak = 0
                    plan = graphs[i].plan(int(roots[i]), b, acc, t, gens[i])
                    failed[i] = graphs[i].queue_peak > cap
                if failed[i]:
                    assert out["status"][i] == native.MP_ERR_ALLOC and out["plan_len"][i] == 0 and (out["plans"][i] == -1).all(), (call, i)
                else:
                    assert out["status"][i] == 0, (call, i)
                    assert out["plans"][i, :out["plan_len"][i]].tolist() == plan, (call, i)
                    assert np.array_equal(rng[i], native.rng_state_from_generator(gens[i])), (call, i)
                    assert gr.same_listing(handle.export(i), graphs[i].listing()) == [], (call, i)
            assert failed == [False, True, False], call
        handle.close()
        model.close()
    finally:
        ctx.close()
    env = env_of(tab, 8)
    agent = agent_factory(env, golden_config(case))
    agent.planner.queue_capacity = cap
    agent.seed(int(case["seed"]))
    with pytest.raises(RuntimeError, match="queue_capacity"):
        agent.act(8)
    with pytest.raises(RuntimeError, match="queue_capacity"):      # and again: the planner stays failed
        agent.act(8)


def test_model_kinds_that_are_refused():
    ctx = native.Context(0)
    try:
        dense = generators.random_stochastic(10, 3, seed=1)
        sparse = generators.random_sparse(10, 3, 2, seed=2)
        det = generators.random_deterministic(10, 3, seed=3)
        models = [ctx.load_dense(dense["transition"], dense["reward"], dense["terminal"]),
                  ctx.load_sparse(sparse["transition"], sparse["next"], sparse["reward"], sparse["terminal"]),
                  ctx.load_joint(np.stack([det["transition"]] * 2), np.stack([det["reward"]] * 2)),
                  ctx.load_table_batch(np.stack([det["transition"]] * 2), np.stack([det["reward"]] * 2))]
        for model in models:
            with pytest.raises(native.NativeError) as e:
                native.GraphBasedPlanners(ctx, model, 2)
            assert e.value.code == native.MP_ERR_MODE
            model.close()
    finally:
        ctx.close()
    env = FiniteMDPEnv(dict(generators.random_stochastic(10, 3, seed=1), mode="stochastic"))
    env.reset()
    with pytest.raises(TypeError):
        agent_factory(env, {"__class__": GBOPD_AGENT}).act(0)


def test_tables_that_change_under_a_kept_graph_are_refused():
    """Bounds, parents and counters were built on the previous tables: the library refuses the next plan and the export with
    the reason, and the agent raises it (an environment whose MDP edits its rows in place keeps its device model)."""
    tab = generators.random_deterministic(40, 4, seed=77)
    ctx = native.Context(0)
    try:
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        handle = native.GraphBasedPlanners(ctx, model, 2)
        rng = native.seed_sequence_states((), 9, 2)
        assert (handle.plan([0, 1], 40, 0.8, 1 / (1 - 0.8), 1e-2, 20, rng)["status"] == 0).all()
        handle.export(0)
        model.set_available(generators.random_available(40, 4, seed=78, rate=0.4))
        for call in (lambda: handle.plan([0, 1], 40, 0.8, 1 / (1 - 0.8), 1e-2, 20, rng), lambda: handle.export(0)):
            with pytest.raises(native.NativeError, match="kept graph") as e:
                call()
            assert e.value.code == native.MP_ERR_ARG
        handle.close()
        fresh = native.GraphBasedPlanners(ctx, model, 2)             # new planners on the new tables are fine
        assert (fresh.plan([0, 1], 40, 0.8, 1 / (1 - 0.8), 1e-2, 20, rng)["status"] == 0).all()
        fresh.close()
        model.close()
    finally:
        ctx.close()
    env = env_of(tab, 0)
    agent = agent_factory(env, {"__class__": GBOPD_AGENT, "budget": 40})
    agent.act(0)
    model = agent.planner._device[0]
    env.mdp.edit_rows([1], reward=np.asarray(tab["reward"])[1:2] * 0.5)
    with pytest.raises(NotImplementedError, match="previous tables"):
        agent.act(0)
    assert agent.planner._device[0] is model                          # (the same device model, patched row by row)
    agent.planner.forget()
    agent.act(0)


def test_a_plan_that_does_not_converge_is_ended(monkeypatch):
    """The pop limit of a plan (2^22; with accuracy 0 and rewards outside [0, 1] the reference may never return), lowered
    through MP_GBOPD_MAX_POPS so that both outcomes are asserted on a plan whose pops the restatement counts: under the
    limit the plan equals the restatement; at it, the planner reports MP_ERR_GBOPD_DIVERGED with exactly the limit's pops
    applied, stays failed, the other planner of the batch is untouched, and the agent raises RuntimeError."""
    tab = generators.random_deterministic(30, 3, seed=79)
    cfg = dict(budget=90, gamma=0.9, accuracy=1e-3, sampling_timeout=50)
    graphs = [gr.Graph(tab["transition"], tab["reward"], 0.9) for _ in range(2)]
    rng = native.seed_sequence_states((), 11, 2)
    roots = [7, 0]
    for i in range(2):
        graphs[i].plan(roots[i], 90, 1e-3, 50, generator_from(rng[i]))
    assert graphs[0].pops > graphs[1].pops + 2, (graphs[0].pops, graphs[1].pops)
    limit = (graphs[0].pops + graphs[1].pops) // 2                  # planner 0 hits it, planner 1 does not
    ctx = native.Context(0)
    try:
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        monkeypatch.setenv("MP_GBOPD_MAX_POPS", str(graphs[0].pops))      # exactly enough: nothing is refused
        handle = native.GraphBasedPlanners(ctx, model, 2)
        out = handle.plan(roots, 90, 0.9, 1 / (1 - 0.9), 1e-3, 50, rng.copy())
        assert (out["status"] == 0).all() and out["updates"].tolist() == [g.pops for g in graphs]
        for i in range(2):
            assert gr.same_listing(handle.export(i), graphs[i].listing()) == [], i
        handle.close()
        monkeypatch.setenv("MP_GBOPD_MAX_POPS", str(limit))
        handle = native.GraphBasedPlanners(ctx, model, 2)
        out = handle.plan(roots, 90, 0.9, 1 / (1 - 0.9), 1e-3, 50, rng.copy())
        assert out["status"].tolist() == [native.MP_ERR_GBOPD_DIVERGED, 0]
        assert int(out["updates"][0]) == limit and out["plan_len"][0] == 0
        assert gr.same_listing(handle.export(1), graphs[1].listing()) == []
        monkeypatch.delenv("MP_GBOPD_MAX_POPS")
        again = handle.plan(roots, 3, 0.9, 1 / (1 - 0.9), 1e-3, 50, rng.copy())
        assert again["status"].tolist() == [native.MP_ERR_GBOPD_DIVERGED, 0]
        handle.close()
        model.close()
    finally:
        ctx.close()
    monkeypatch.setenv("MP_GBOPD_MAX_POPS", str(limit))
    agent = agent_factory(env_of(tab, roots[0]), dict(cfg, __class__=GBOPD_AGENT))
    native.generator_set_state(agent.planner.np_random, rng[0])
    with pytest.raises(RuntimeError, match="without converging"):
        agent.act(roots[0])


def test_a_node_without_a_listed_action_cannot_reach_the_planner():
    """np.amax([]) in partial_value_iteration (graph_based.py:74) needs a state that lists no action.  The library refuses
    such an availability table when it is set, as the project's environments do, so MP_ERR_GBOPD_NO_ACTION is a guard the
    kernel keeps for tables it cannot vouch for; the planner maps it to the reference's ValueError."""
    from rl_agents_amd.agents.tree_search.graph_based import GraphBasedPlanner
    tab = generators.random_deterministic(12, 3, seed=80)
    avail = np.ones((12, 3), bool)
    avail[int(tab["transition"][0, 0])] = False
    ctx = native.Context(0)
    try:
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        with pytest.raises(native.NativeError):
            model.set_available(avail)
        model.close()
    finally:
        ctx.close()
    with pytest.raises(ValueError, match="zero-size array"):
        GraphBasedPlanner.raise_for_status(np.asarray([0, native.MP_ERR_GBOPD_NO_ACTION]))
