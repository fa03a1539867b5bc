"""MDP-GapE on the device (mp_gape_plan, rl_agents_amd/csrc/gape.hip) against the reference's own outputs
(tests/golden/gape.npz, tests/golden/kl_lower_bound.npz) and the test-side restatement (tests/gape_restatement.py).

Parity: plans, episodes run, env steps, status or exception, generator records and the tree's structure, counts, cumulative
rewards and done flags exactly; mu_ucb / mu_lcb / value_upper / value_lower within 1e-12 / (1 - gamma) (the device's log in
the Newton steps: 1e-12 a bound, and a value sums at most 1 / (1 - gamma) of them)."""
import os

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, generators
from tests import gape_restatement as gr
from tests.helpers import assert_form
from tests.test_gape_host import ERRORS, GAPE_AGENT, GOLDEN, HERE, golden_case, names, restate
from tests.test_gpu_olop import golden_env

pytestmark = pytest.mark.gpu

BOUND_TOL = 1e-12
EXACT = ("parent", "kind", "action", "depth", "count", "done", "cum")
BOUNDS = ("mu_ucb", "mu_lcb", "vu", "vl")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def agent_config(case):
    return dict(gamma=float(case["gamma"]), episodes=int(case["episodes"]), horizon=int(case["horizon"]), budget=int(case["budget"]),
                accuracy=float(case["accuracy"]), confidence=float(case["confidence"]), continuation_type=str(case["continuation"]),
                upper_bound=dict(type="kullback-leibler", threshold=str(case["threshold"])))


def golden_agent(case):
    env = golden_env(dict(case, max_steps=0))
    agent = agent_factory(env, dict(agent_config(case), __class__=GAPE_AGENT))
    native.generator_set_state(agent.planner.np_random, case["rng_before"])
    return env, agent


def assert_tree(tree, ref, gamma, name):
    for k in EXACT:
        assert np.array_equal(tree[k], ref[k]), (name, k)
    for k in BOUNDS:
        err = np.abs(np.asarray(tree[k]) - np.asarray(ref[k]))
        assert np.all(err <= BOUND_TOL / (1 - gamma)), (name, k, err.max())


def test_lower_bound_on_the_device_against_the_reference(ctx):
    g = np.load(os.path.join(HERE, "golden", "kl_lower_bound.npz"))
    out, its, mask = ctx.selftest_olop_bound("kl_lower_bound", g["total"], g["threshold"], g["count"])
    err = np.abs(out - g["bound"])
    print("kl_lower_bound: max |device - reference| =", err.max())
    assert np.all(err <= BOUND_TOL), err.max()
    assert np.array_equal(its, g["iterations"]) and np.array_equal(mask, g["decisions"])
    assert np.all(out >= 0) and np.all(out * g["count"] <= g["total"] * (1 + 1e-15))      # on [0, mu]


def test_every_golden_case_through_the_c_abi(z):
    planned = 0
    for name in names(z):
        case = golden_case(z, name)
        if str(case["error"]) == "ZeroDivisionError":
            continue                                     # the host's eval raises: nothing reaches the library
        env, agent = golden_agent(case)
        planner = agent.planner
        model, order = planner.model_for(env), case["order"]
        column = np.empty(len(order), np.int32)
        column[order] = np.arange(len(order))
        rng = case["rng_before"].reshape(1, 6).copy()
        out = planner.models.ctx.gape_plan(model, [int(case["s0"])], int(case["episodes"]), int(case["horizon"]),
                                           float(case["gamma"]), float(case["accuracy"]), str(case["continuation"]) == "uniform",
                                           len(order), column, planner.thresholds(), planner._value_init, rng)
        assert_form(planner.models.ctx, "gape_global")
        assert np.array_equal(rng[0], case["rng_after"]), name
        assert int(out["env_steps"][0]) == int(case["env_steps"]), name
        if str(case["error"]):
            want = native.ERR_GAPE_NO_CHALLENGER if name == "one_action" else native.MP_ERR_REWARD_RANGE
            assert int(out["status"][0]) == want and int(out["plan_len"][0]) == 0 and int(out["plans"][0, 0]) == -1, name
            continue
        assert int(out["status"][0]) == native.MP_OK and int(out["plan_len"][0]) == 1, name
        assert int(order[out["plans"][0, 0]]) == int(case["plan"][0]) == int(order[out["best_challenger"][0, 0]]), name
        assert int(out["episodes_run"][0]) == int(case["episodes_run"]), name
        assert int(out["env_steps"][0]) == int(case["episodes_run"]) * int(case["horizon"]), name
        tree = planner.models.ctx.gape_tree(0)
        chance = tree["kind"] == 1
        tree["action"] = np.where(chance, order[np.clip(tree["action"], 0, len(order) - 1)], tree["action"]).astype(np.int32)
        ref = {k: case["tree/" + k] for k in EXACT + BOUNDS}
        assert_tree(gr.as_bfs(tree), ref, float(case["gamma"]), name)
        # the root's arms as the call reports them: the tree's depth-0 chance nodes, by column
        arms = np.flatnonzero(chance & (tree["parent"] == 0))
        cols = column[tree["action"][arms]]
        assert np.array_equal(out["child_count"][0, cols], tree["count"][arms]), name
        assert np.array_equal(out["child_upper"][0, cols], tree["vu"][arms]), name
        assert np.array_equal(out["child_lower"][0, cols], tree["vl"][arms]), name
        assert (np.delete(out["child_count"][0], cols) == -1).all(), name
        planned += 1
    assert planned >= 13


def test_every_golden_case_through_the_agent(z):
    planned = 0
    for name in names(z):
        case = golden_case(z, name)
        env, agent = golden_agent(case)
        if str(case["error"]):
            with pytest.raises(ERRORS[str(case["error"])], match=str(case["message"])[:20].replace("(", r"\(").replace(")", r"\)")):
                agent.plan(int(case["s0"]))
            # the draws and steps made before the reference raised
            assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
            assert agent.planner.env_steps == int(case["env_steps"]), name
            continue
        assert agent.plan(int(case["s0"])) == case["plan"].tolist(), name
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
        assert agent.planner.env_steps == int(case["env_steps"]), name
        assert agent.planner.budget_used == int(case["episodes_run"]) * int(case["horizon"]), name
        assert agent.planner.get_plan() == case["plan"].tolist(), name
        # the linked tree, listed as the golden file lists the reference's
        root = agent.planner.root
        nodes, parents = [root], [-1]
        i = 0
        while i < len(nodes):
            for c in nodes[i].children.values():
                nodes.append(c)
                parents.append(i)
            i += 1
        from rl_agents_amd.agents.tree_search.mdp_gape import ChanceNode
        dec = [not isinstance(n, ChanceNode) for n in nodes]
        tree = dict(parent=np.asarray(parents), kind=np.asarray([0 if d else 1 for d in dec]),
                    action=np.asarray([-1 if n.parent is None else int(n.action) for n in nodes]),
                    depth=np.asarray([n.depth for n in nodes]), count=np.asarray([n.count for n in nodes]),
                    done=np.asarray([int(n.done) if d else 0 for n, d in zip(nodes, dec)]),
                    cum=np.asarray([n.cumulative_reward if d else 0.0 for n, d in zip(nodes, dec)]),
                    mu_ucb=np.asarray([n.mu_ucb if d else 0.0 for n, d in zip(nodes, dec)]),
                    mu_lcb=np.asarray([n.mu_lcb if d else 0.0 for n, d in zip(nodes, dec)]),
                    vu=np.asarray([n.value_upper for n in nodes]), vl=np.asarray([n.value_lower for n in nodes]))
        assert_tree(tree, {k: case["tree/" + k] for k in EXACT + BOUNDS}, float(case["gamma"]), name)
        assert root.selection_rule() == int(case["plan"][0]), name
        visits = agent.planner.get_visits()
        assert sum(visits.values()) == int(case["env_steps"]), name
        planned += 1
    assert planned >= 13


SMALL = generators.random_deterministic(12, 3, seed=82)
SMALL_CFG = dict(horizon=3, episodes=30, gamma=0.8, accuracy=2.1)   # (values reach 2.44: some plans stop early, some run out)


def small_env(s0=0):
    env = FiniteMDPEnv(dict(mode="deterministic", transition=SMALL["transition"].tolist(), reward=SMALL["reward"].tolist(),
                            terminal=SMALL["terminal"].astype(int).tolist(), state=int(s0)))
    env.reset()
    return env


def small_case(s0, rng6):
    planner_cfg = dict(SMALL_CFG, confidence=0.9, continuation="uniform", threshold=gr.DEFAULT_THRESHOLD)
    return dict({"mdp/" + k: np.asarray(SMALL[k]) for k in ("transition", "reward", "terminal")}, s0=s0, rng_before=rng6,
                available=np.ones((12, 3), bool), order=np.arange(3), done_on_next=False, **planner_cfg)


@pytest.mark.parametrize("n", [1, 2, 65])
def test_a_batch_equals_its_single_root_calls(n):
    env = small_env()
    agent = agent_factory(env, dict(SMALL_CFG, __class__=GAPE_AGENT))
    agent.seed(7)
    roots = (np.arange(n) * 5 % 12).astype(np.int32)
    rng = agent.planner.batch_rng_states(n)
    assert len({r.tobytes() for r in rng}) == n
    rng0 = rng.copy()
    out = agent.planner.plan_batch(env, roots, rng_states=rng)
    assert_form(agent.planner.models.ctx, "gape_global")
    trees = {i: agent.planner.models.ctx.gape_tree(i) for i in (0, n - 1)}
    for i in range(n):
        one = rng0[i:i + 1].copy()
        single = agent.planner.plan_batch(env, roots[i:i + 1], rng_states=one)
        for k in ("plans", "plan_len", "episodes_run", "env_steps", "status", "child_lower", "child_upper", "child_count",
                  "best_challenger"):
            assert np.array_equal(out[k][i], single[k][0]), (i, k)
        assert np.array_equal(rng[i], one[0]), i
        if i in trees:
            tree = agent.planner.models.ctx.gape_tree(0)
            assert all(np.array_equal(tree[k], trees[i][k]) for k in tree), i


def test_300_roots_against_the_restatement():
    """The discrete results only: plans, both arms, episodes run, env steps, counts of the root's arms, generator records."""
    env = small_env()
    agent = agent_factory(env, dict(SMALL_CFG, __class__=GAPE_AGENT))
    agent.seed(11)
    n = 300
    roots = (np.arange(n) % 12).astype(np.int32)
    rng = agent.planner.batch_rng_states(n)
    rng0 = rng.copy()
    out = agent.planner.plan_batch(env, roots, rng_states=rng)
    assert (out["status"] == native.MP_OK).all()
    stopped_early = 0
    for i in range(n):
        res, gen = restate(small_case(int(roots[i]), rng0[i]))
        assert out["plans"][i].tolist() == res["plan"].tolist(), i
        assert out["best_challenger"][i].tolist() == [res["best"], res["challenger"]], i
        assert int(out["episodes_run"][i]) == res["episodes_run"] and int(out["env_steps"][i]) == res["env_steps"], i
        assert np.array_equal(rng[i], native.rng_state_from_generator(gen)), i
        arms = np.flatnonzero((res["kind"] == 1) & (res["parent"] == 0))
        assert np.array_equal(out["child_count"][i, res["action"][arms]], res["count"][arms]), i
        stopped_early += res["episodes_run"] < SMALL_CFG["episodes"] + 2
    assert 0 < stopped_early < n, "both ends of the plan loop are part of the case"


def test_more_trees_than_the_workspace_keeps():
    """40 000 roots of 289 records each pass 1 GiB: the workgroups share slots and only root 0's tree is kept."""
    env = small_env()
    agent = agent_factory(env, dict(SMALL_CFG, __class__=GAPE_AGENT))
    agent.seed(13)
    n = 40000
    roots = (np.arange(n) % 12).astype(np.int32)
    rng = agent.planner.batch_rng_states(n)
    rng0 = rng.copy()
    out = agent.planner.plan_batch(env, roots, rng_states=rng)
    assert_form(agent.planner.models.ctx, "gape_global_slots")
    assert (out["status"] == native.MP_OK).all()
    for i in (0, 1, 255, 256, 8192, 8193, 20001, n - 1):       # (root 0's own slot, first and later rounds of a workgroup)
        res, gen = restate(small_case(int(roots[i]), rng0[i]))
        assert out["plans"][i].tolist() == res["plan"].tolist(), i
        assert out["best_challenger"][i].tolist() == [res["best"], res["challenger"]], i
        assert int(out["episodes_run"][i]) == res["episodes_run"] and int(out["env_steps"][i]) == res["env_steps"], i
        assert np.array_equal(rng[i], native.rng_state_from_generator(gen)), i
    res, _ = restate(small_case(int(roots[0]), rng0[0]))
    tree = agent.planner.models.ctx.gape_tree(0)
    for k in EXACT:
        assert np.array_equal(tree[k], res[k]), k
    with pytest.raises(native.NativeError, match="only root 0"):
        agent.planner.models.ctx.gape_tree(1)


def test_tree_plot_reads_the_exported_tree():
    from rl_agents_amd.agents.tree_search.graphics import TreePlot
    from rl_agents_amd.agents.tree_search.mdp_gape import ChanceNode, DecisionNode
    env = small_env(3)
    agent = agent_factory(env, dict(SMALL_CFG, __class__=GAPE_AGENT))
    agent.seed(5)
    action = agent.act(3)
    root = agent.planner.root
    assert isinstance(root, DecisionNode) and all(isinstance(c, ChanceNode) for c in root.children.values())
    assert root.selection_rule() == action and set(root.children) == {0, 1, 2}
    plot = TreePlot(agent.planner, max_depth=4)
    assert plot.total_count == sum(c.count for c in root.children.values()) == agent.planner.budget_used // 3
    assert len(plot.segments()) == sum(1 for c in root.children.values() if c.count)


def test_batched_evaluation_runs_the_agent_through_plan_batch():
    """The host-stepped loop of BatchedEvaluation, 4 episodes, against four sequential agent / env loops."""
    from rl_agents_amd.trainer.batched_evaluation import BatchedEvaluation
    cfg = dict(mode="deterministic", transition=SMALL["transition"].tolist(), reward=SMALL["reward"].tolist(),
               terminal=SMALL["terminal"].astype(int).tolist(), state=2, max_steps=5)
    env = FiniteMDPEnv(cfg)
    env.reset()
    acfg = dict(SMALL_CFG, __class__=GAPE_AGENT)
    ev = BatchedEvaluation(env, agent_factory(env, dict(acfg)), num_episodes=4, sim_seed=40)
    assert not ev._device_capable()
    out = ev.run()
    assert out["device_resident"] is False
    for i in range(4):
        e = FiniteMDPEnv(cfg)
        e.reset()
        agent = agent_factory(e, dict(acfg))
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


def test_refusals_of_the_entry_point():
    env = small_env()
    agent = agent_factory(env, dict(SMALL_CFG, __class__=GAPE_AGENT))
    planner = agent.planner
    model = planner.model_for(env)
    thr, vin = planner.thresholds(), planner._value_init
    rng = planner.batch_rng_states(1)

    def call(model=model, episodes=30, horizon=3, thr=thr, vin=vin):
        return planner.models.ctx.gape_plan(model, [0], episodes, horizon, 0.8, 1.0, True, 3, None, thr, vin, rng)
    # the node bound 1 + (episodes + 2) * horizon * 3 at the longest horizon: 14.8 M records of 104 bytes; 2.15 G records
    long_init = np.ones(16384 + 1)
    with pytest.raises(native.NativeError, match="1 GiB"):
        call(episodes=300, horizon=16384, thr=np.ones(302), vin=long_init)
    with pytest.raises(native.NativeError, match="32-bit"):
        call(episodes=43700, horizon=16384, thr=np.ones(43702), vin=long_init)
    # tables that are not finite are refused on the host, before anything is launched
    for bad in (np.nan, np.inf):
        spoiled = thr.copy()
        spoiled[5] = bad
        with pytest.raises(native.NativeError, match="threshold of count 6 is not finite") as e:
            call(thr=spoiled)
        assert e.value.code == native.MP_ERR_ARG
        spoiled = vin.copy()
        spoiled[1] = bad
        with pytest.raises(native.NativeError, match="initial value of depth 1 is not finite"):
            call(vin=spoiled)
    for gamma, accuracy in ((np.nan, 1.0), (0.8, np.nan), (np.inf, 1.0)):
        with pytest.raises(native.NativeError, match="gamma and accuracy must be finite"):
            planner.models.ctx.gape_plan(model, [0], 30, 3, gamma, accuracy, True, 3, None, thr, vin, rng)
    assert np.array_equal(rng, planner.batch_rng_states(1))              # no refusal touched the generator record
    # the agent refuses the same before the call: "confidence": 1.5 makes np.log of a negative number, a NaN and a warning
    nan_agent = agent_factory(env, dict(SMALL_CFG, __class__=GAPE_AGENT, confidence=1.5))
    with np.errstate(invalid="ignore"), pytest.raises(ValueError, match="must be finite"):
        nan_agent.plan(0)
    assert nan_agent.planner.env_steps == 0
    for other in (generators.random_stochastic(10, 3, seed=2), generators.random_sparse(10, 3, 2, seed=3)):
        from rl_agents_amd import device_model
        m = planner.models.get(device_model.spec_from_mdp(device_model.finite_mdp_of(FiniteMDPEnv(dict(other)))))
        with pytest.raises(native.NativeError) as e:
            call(model=m)
        assert e.value.code == native.MP_ERR_MODE
    with pytest.raises(native.NativeError, match="no tree of mp_gape_plan"):
        planner.models.ctx.olop_plan(model, [0], 4, 2, 0.8, True, -1, np.ones(4), np.ones(3), rng)
        planner.models.ctx.gape_tree(0)
