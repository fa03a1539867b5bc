"""OLOP / KL-OLOP on the device (mp_olop_plan, rl_agents_amd/csrc/olop.hip) against the reference's own outputs
(tests/golden/olop.npz) and the test-side restatement (tests/olop_restatement.py).

Parity: plans, tree shapes, actions, counts, done flags, cumulative rewards, generator records and env-step counts exactly;
mu_ucb / value_upper within 1e-12 (the device's log in the KL bound's Newton step)."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv, generators
from tests import olop_restatement as olr
from tests.helpers import assert_form
from tests.test_olop_host import GOLDEN, OLOP_AGENT, generator_from, golden_case, names

pytestmark = pytest.mark.gpu

BOUND_TOL = 1e-12


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def env_of(transition, reward, terminal, s0, available=None, order=None, max_steps=0, done_rule="source"):
    cfg = dict(mode="deterministic", transition=np.asarray(transition).tolist(), reward=np.asarray(reward).tolist(),
               terminal=np.asarray(terminal).astype(int).tolist(), state=int(s0), max_steps=int(max_steps), done_rule=done_rule)
    if available is not None and order is not None and not np.array_equal(order, np.arange(len(order))):
        env = OrderedMaskedFiniteMDPEnv(dict(cfg, available=np.asarray(available).astype(int).tolist(),
                                             listing_order=[int(a) for a in order]))
    elif available is not None and not np.asarray(available).all():
        env = MaskedFiniteMDPEnv(dict(cfg, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(cfg)
    env.reset()
    return env


def golden_env(case):
    return env_of(case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"], int(case["s0"]), case["available"],
                  case["order"], int(case["max_steps"]), "next" if bool(case["done_on_next"]) else "source")


def agent_config(case):
    cfg = dict(gamma=float(case["gamma"]), continuation_type=str(case["continuation"]),
               upper_bound=dict(type=str(case["bound_type"])))
    if str(case["bound_time"]):
        cfg["upper_bound"]["time"] = str(case["bound_time"])
    if str(case["threshold"]):
        cfg["upper_bound"]["threshold"] = str(case["threshold"])
    cfg["episodes"], cfg["horizon"] = int(case["episodes"]), int(case["horizon"])
    return cfg


def assert_tree(tree, ref, name):
    for k in ("parent", "action", "depth", "count", "done"):
        assert np.array_equal(tree[k], ref[k]), (name, k)
    assert np.array_equal(tree["cum"], ref["cum"]), (name, "cum")
    for k in ("mu", "vu"):
        a, b = np.asarray(tree[k]), np.asarray(ref[k])
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), (name, k)
        fin = np.isfinite(b)
        assert np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), (name, k)
        assert np.all(np.abs(a[fin] - b[fin]) <= BOUND_TOL), (name, k, np.abs(a[fin] - b[fin]).max())


def export_arrays(planner):
    root = planner.root
    nodes, parents = [root], [-1]
    i = 0
    while i < len(nodes):
        for c in nodes[i].children.values():
            nodes.append(c)
            parents.append(i)
        i += 1
    return dict(parent=np.asarray(parents, np.int32), action=np.asarray([n.action if n.parent else -1 for n in nodes], np.int32),
                depth=np.asarray([n.depth for n in nodes], np.int32), count=np.asarray([n.count for n in nodes], np.int64),
                cum=np.asarray([n.cumulative_reward for n in nodes]), mu=np.asarray([n.mu_ucb for n in nodes]),
                vu=np.asarray([n.value_upper for n in nodes]), done=np.asarray([n.done for n in nodes], np.uint8))


def golden_cases_through_the_agent(z):
    """Every case of a golden file in the layout of olop.npz through OLOPAgent; returns how many plans were compared."""
    checked = 0
    for name in names(z):
        case = golden_case(z, name)
        if str(case["error"]) and str(case["at"]) == "construction":
            continue
        env = golden_env(case)
        agent = agent_factory(env, dict(agent_config(case), __class__=OLOP_AGENT))
        native.generator_set_state(agent.planner.np_random, case["rng_before"])
        if str(case["error"]):
            with pytest.raises({"KeyError": KeyError, "ValueError": ValueError}[str(case["error"])]):
                agent.plan(int(case["s0"]))
            # the draws and steps made before the reference raised
            assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
            assert agent.planner.env_steps == int(case["env_steps"]), name
            continue
        plan = agent.plan(int(case["s0"]))
        assert plan == case["plan"].tolist(), name
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
        assert agent.planner.env_steps == int(case["env_steps"]), name
        ref = {k: case["tree/" + k] for k in ("parent", "action", "depth", "count", "cum", "mu", "vu", "done")}
        assert_tree(export_arrays(agent.planner), ref, name)
        visits = agent.planner.get_visits()
        assert sorted(visits) == [str(k) for k in case["visit_keys"]], name
        assert [visits[str(k)] for k in case["visit_keys"]] == case["visit_counts"].tolist(), name
        checked += 1
    return checked


def test_every_golden_case(z):
    assert golden_cases_through_the_agent(z) >= 15


def test_act_episode_through_agent_factory(z):
    """A reference KL-OLOP config (GridWorld/agents/kl-olop.json) with only its __class__ line changed."""
    cfg = {"__class__": OLOP_AGENT, "gamma": 0.8, "budget": 500, "max_depth": 4,
           "upper_bound": {"type": "kullback-leibler", "c": 2}, "lazy_tree_construction": True, "continuation_type": "uniform"}
    env = env_of(z["olop_episode/mdp/transition"], z["olop_episode/mdp/reward"], z["olop_episode/mdp/terminal"], 0)
    agent = agent_factory(env, cfg)
    agent.seed(int(z["olop_episode/seed"]))
    assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), z["olop_episode/rng_before"])
    for t in range(len(z["olop_episode/actions"])):
        assert env.mdp.state == int(z["olop_episode/states"][t])
        a = agent.act(env.mdp.state)
        assert a == int(z["olop_episode/actions"][t]), t
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), z["olop_episode/rng_after"][t]), t
        env.step(a)


def restated_root(tr, rw, term, s0, cfg, rng6, available=None, order=None):
    kl = cfg["upper_bound"]["type"] == "kullback-leibler"
    thr = olr.thresholds(cfg["upper_bound"].get("threshold", "4*np.log(time)"), cfg["upper_bound"].get("time", "global"),
                         cfg["episodes"]) if kl else None
    gen = generator_from(rng6)
    res = olr.olop_plan(tr, rw, term, int(s0), cfg["episodes"], cfg["horizon"], cfg["gamma"], kl, thr,
                        cfg.get("continuation_type", "zeros"), gen, available=available, order=order)
    return res, native.rng_state_from_generator(gen)


def check_batch(env, cfg, roots, sample, available=None, order=None, tree_roots=(), form="olop_global"):
    agent = agent_factory(env, dict(cfg, __class__=OLOP_AGENT))
    pc = agent.planner.config
    rng = agent.planner.batch_rng_states(len(roots))
    rng0 = rng.copy()
    out = agent.planner.plan_batch(env, roots, rng_states=rng)
    assert_form(agent.planner.models.ctx, form)
    mdp = env.mdp
    ref_cfg = dict(pc)
    for i in sample:
        res, rng_after = restated_root(mdp.transition, mdp.reward, mdp.terminal, roots[i], ref_cfg, rng0[i], available, order)
        n = int(out["plan_len"][i])
        assert out["plans"][i, :n].tolist() == res["plan"].tolist(), i
        assert np.array_equal(rng[i], rng_after), i
        assert int(out["env_steps"][i]) == res["env_steps"] == pc["episodes"] * pc["horizon"], i
        if not np.isfinite(res["vu"][0]):
            assert np.array_equal(out["root_value"][i], res["vu"][0], equal_nan=True), i
        else:
            assert abs(out["root_value"][i] - res["vu"][0]) <= BOUND_TOL, i
        if i in tree_roots:
            tree = agent.planner.models.ctx.olop_tree(i, 1 + pc["episodes"] * pc["horizon"] * mdp.reward.shape[1])
            tree = agent.planner.relabel_tree(tree, agent.planner._last_model)
            assert_tree(tree, res, i)
    return out


@pytest.mark.parametrize("n", [1, 256, 4096, 65536])
def test_batches_against_the_restatement(n):
    """A tree per root, kept for the export, while the batch's trees fit 1 GiB (olop_global); 65 536 roots share the slots of the
    resident wavefronts (olop_global_slots: only root 0's tree is kept)."""
    grid = generators.gridworld()
    env = env_of(grid["transition"], grid["reward"], grid["terminal"], 0)
    cfg = {"gamma": 0.8, "budget": 500, "upper_bound": {"type": "kullback-leibler"}, "continuation_type": "uniform"}
    roots = (np.arange(n) * 37 % 100).astype(np.int32)
    sample = sorted({0, n - 1, n // 2, n // 3, (7 * n) // 9})
    check_batch(env, cfg, roots, sample, tree_roots=(0, n - 1) if n <= 4096 else (0,),
                form="olop_global" if n <= 4096 else "olop_global_slots")


def test_highway_shaped_batch_with_restricted_actions():
    hw = generators.highway_shaped(4, 5, 20, seed=5)
    s = hw["reward"].shape[0]
    avail = generators.random_available(s, 5, seed=6, rate=0.3)
    order = [1, 0, 2, 3, 4]
    env = env_of(hw["transition"], np.clip(hw["reward"], 0, 1), hw["terminal"], 0, avail, order)
    cfg = {"gamma": 0.7, "budget": 300, "upper_bound": {"type": "kullback-leibler", "threshold": "2*np.log(time)"},
           "continuation_type": "uniform"}
    roots = (np.arange(512) * 13 % s).astype(np.int32)
    check_batch(env, cfg, roots, [0, 1, 100, 511], available=avail, order=order, tree_roots=(0, 100))


def test_fuzz_against_the_restatement():
    rng = np.random.default_rng(1234)
    for case in range(40):
        S, A = int(rng.integers(2, 40)), int(rng.integers(1, 9))
        tab = generators.random_deterministic(S, A, seed=1000 + case, terminal_rate=float(rng.choice([0.0, 0.2, 0.5])))
        if rng.random() < 0.3:
            tab["reward"] = (tab["reward"] > 0.5).astype(np.float64)
        gamma = float(rng.choice([0.5, 0.7, 0.8, 0.9, 0.95]))
        budget = int(rng.integers(20, 400))       # (smaller budgets with gamma 0.5 cannot be split: ValueError, olop.py:61)
        bound = {"type": str(rng.choice(["kullback-leibler", "kullback-leibler", "hoeffding"])),
                 "time": str(rng.choice(["global", "local"]))}
        cont = "uniform" if (rng.random() < 0.6 or A == 1) else "zeros"
        available = order = None
        if A > 1 and rng.random() < 0.4:
            available = generators.random_available(S, A, seed=2000 + case, rate=0.3)
            if cont == "zeros":
                available[:, 0] = True
            order = list(rng.permutation(A)) if rng.random() < 0.5 else list(range(A))
        env = env_of(tab["transition"], tab["reward"], tab["terminal"], 0, available, order)
        cfg = {"gamma": gamma, "budget": budget, "upper_bound": bound, "continuation_type": cont}
        n = int(rng.integers(1, 70))
        roots = rng.integers(0, S, size=n).astype(np.int32)
        check_batch(env, cfg, roots, range(n), available=available, order=order, tree_roots=(0,))


def test_batched_evaluation_equals_sequential_agents():
    from rl_agents_amd.agents.tree_search.olop import OLOPAgent
    from rl_agents_amd.trainer.batched_evaluation import BatchedEvaluation
    tab = generators.random_deterministic(30, 3, seed=77, terminal_rate=0.15)
    cfg = dict(tab, state=2, max_steps=8)
    env = FiniteMDPEnv(cfg)
    env.reset()
    agent_cfg = dict(budget=120, gamma=0.9, upper_bound={"type": "kullback-leibler"}, continuation_type="uniform")
    out = BatchedEvaluation(env, OLOPAgent(env, dict(agent_cfg)), num_episodes=6, sim_seed=40).run()
    for i in range(6):
        e = FiniteMDPEnv(cfg)
        e.reset()
        agent = OLOPAgent(e, dict(agent_cfg))
        agent.seed(40 + i)
        actions, total, done = [], 0.0, False
        while not done:
            a = agent.act(e.mdp.state)
            _, r, term, trunc, _ = e.step(a)
            actions.append(a)
            total += r
            done = term or trunc
        assert out["lengths"][i] == len(actions)
        np.testing.assert_array_equal(out["actions"][i, :len(actions)], actions)
        assert out["returns"][i] == pytest.approx(total, abs=1e-12)


def test_errors():
    bad = generators.random_deterministic(20, 3, seed=45)
    bad["reward"][:, 1] = -0.5
    env = env_of(bad["transition"], bad["reward"], bad["terminal"], 0)
    agent = agent_factory(env, {"__class__": OLOP_AGENT, "budget": 100, "continuation_type": "uniform",
                                "upper_bound": {"type": "kullback-leibler"}})
    with pytest.raises(ValueError):
        agent.plan_batch(np.arange(20, dtype=np.int32))
    tab = generators.random_deterministic(20, 3, seed=46)
    avail = np.ones((20, 3), bool)
    avail[5, 0] = False
    env = env_of(tab["transition"], tab["reward"], tab["terminal"], 5, avail)
    agent = agent_factory(env, {"__class__": OLOP_AGENT, "budget": 100})
    with pytest.raises(KeyError):
        agent.act(5)


def test_more_than_64_actions_and_a_horizon_beyond_64():
    """The 64-wide chunks of the kernel: children of an expansion (availability ballot, listing order, the rank of the
    "zeros" action), the selection argmax, the backup max and the plan's count max over |A| = 70; the KL bounds of a path
    of L = 70 nodes."""
    S, A = 40, 70
    tab = generators.random_deterministic(S, A, seed=501, terminal_rate=0.1)
    avail = generators.random_available(S, A, seed=502, rate=0.2)
    avail[:, 0] = True
    order = list(np.random.default_rng(503).permutation(A))
    order.remove(0)
    order.insert(66, 0)                  # action 0 is listed 67th: its device label is past the first chunk
    for cont in ("zeros", "uniform"):
        env = env_of(tab["transition"], tab["reward"], tab["terminal"], 0, avail, order)
        cfg = {"gamma": 0.9, "budget": 400, "upper_bound": {"type": "kullback-leibler"}, "continuation_type": cont}
        roots = (np.arange(40) * 7 % S).astype(np.int32)
        check_batch(env, cfg, roots, range(40), available=avail, order=order, tree_roots=(0, 39))
    long = generators.random_deterministic(25, 3, seed=504, terminal_rate=0.05)
    env = env_of(long["transition"], long["reward"], long["terminal"], 0)
    for bound in ({"type": "kullback-leibler", "time": "local"}, {"type": "hoeffding"}):
        cfg = {"gamma": 0.95, "horizon": 70, "episodes": 6, "upper_bound": bound, "continuation_type": "uniform"}
        roots = np.arange(25, dtype=np.int32)
        check_batch(env, cfg, roots, range(25), tree_roots=(0, 24))


def test_olop_and_stochastic_uct_trees_are_told_apart():
    """mp_olop_tree_export reads only a tree of mp_olop_plan, and mp_uct_stoch_tree_export only one of
    mp_uct_plan_stochastic, whichever planned last on the context."""
    ctx = native.Context(0)
    try:
        tab = generators.random_deterministic(20, 3, seed=7)
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        sp = generators.random_sparse(30, 3, 2, seed=8, terminal_rate=0.1)
        smodel = ctx.load_sparse(sp["transition"], sp["next"], sp["reward"], sp["terminal"])
        p3 = np.ones(3) / 3
        s0 = np.arange(4, dtype=np.int32)

        def olop():
            rng = native.seed_sequence_states((), 1, 4)
            out = ctx.olop_plan(model, s0, 5, 3, 0.8, True, -1, np.full(5, 4 * np.log(5)),
                                np.array([(1 - 0.8 ** (4 - d)) / (1 - 0.8) for d in range(4)]), rng)
            assert (out["status"] == 0).all()

        def stoch():
            rng = native.seed_sequence_states((), 2, 4)
            ctx.uct_plan_stochastic(smodel, s0, 10, 4, 0.9, 5.0, p3, p3, rng, env_rng_state=native.seed_sequence_states((), 3, 4))

        olop()
        assert len(ctx.olop_tree(0, 1 + 5 * 3 * 3)["parent"]) > 1
        with pytest.raises(native.NativeError):
            ctx.uct_stoch_tree(0)
        stoch()
        ctx.uct_stoch_tree(0)
        with pytest.raises(native.NativeError):
            ctx.olop_tree(0, 1 + 5 * 3 * 3)
        olop()
        with pytest.raises(native.NativeError):
            ctx.uct_stoch_tree(0)
        smodel.close()
        model.close()
    finally:
        ctx.close()
