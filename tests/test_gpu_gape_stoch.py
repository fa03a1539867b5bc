"""MDP-GapE with transition bounds on the device (mp_gape_plan_stochastic, rl_agents_amd/csrc/gape_stoch.hip) against the
reference's own outputs (tests/golden/gape_stoch.npz), its single-root calls and mp_gape_plan.

Parity: plans, episodes run, env steps, status or exception, generator records and the tree's structure in the reference's dict
order, counts, cumulative rewards and done flags exactly; mu_ucb / mu_lcb / value_upper / value_lower within
1e-12 / (1 - gamma)."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, generators
from tests import gape_restatement as gr
from tests.helpers import assert_form
from tests.test_gape_stoch_host import (BOUNDS, EXACT, GAPE_AGENT, GOLDEN, STOCH_AGENT, case_agent, golden_case, golden_tree,
                                        names)

pytestmark = pytest.mark.gpu

BOUND_TOL = 1e-12
STATUS = {"placeholders": native.ERR_GAPE_PLACEHOLDERS, "reward_range": native.MP_ERR_REWARD_RANGE}
FORM = {"deterministic": "gape_stoch_table", "stochastic": "gape_stoch_dense", "sparse": "gape_stoch_sparse"}
RESULTS = ("plans", "plan_len", "episodes_run", "env_steps", "status", "child_lower", "child_upper", "child_count", "best_challenger")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def assert_tree(tree, ref, gamma, name):
    for k in EXACT:
        assert np.array_equal(tree[k], ref[k]), (name, k)
    worst = 0.0
    for k in BOUNDS:
        err = np.abs(np.asarray(tree[k]) - np.asarray(ref[k]))
        worst = max(worst, float(err.max()))
        assert np.all(err <= BOUND_TOL / (1 - gamma)), (name, k, err.max())
    return worst


def test_every_golden_case_through_the_c_abi(z):
    planned, worst = 0, 0.0
    for name in names(z):
        case = golden_case(z, name)
        env, agent = case_agent(case)
        planner = agent.planner
        model, order = planner.model_for(env), case["order"]
        column = np.empty(len(order), np.int32)
        column[order] = np.arange(len(order))
        rng = case["rng_before"].reshape(1, 6).copy()
        ctx = planner.models.ctx
        out = ctx.gape_plan_stochastic(model, [int(case["s0"])], int(case["episodes"]), int(case["horizon"]),
                                       int(case["max_next_states_count"]), float(case["gamma"]), float(case["accuracy"]),
                                       str(case["continuation"]) == "uniform", len(order), column, planner.thresholds(),
                                       planner.transition_thresholds(), planner._value_init, rng)
        assert_form(ctx, FORM[str(case["mdp/mode"])])
        assert ctx.last_kernel_variant() in native.gape_stoch_form_names()
        assert np.array_equal(rng[0], case["rng_after"]), name
        assert int(out["env_steps"][0]) == int(case["env_steps"]), name
        if str(case["error"]):
            assert int(out["status"][0]) == STATUS[name] and int(out["plan_len"][0]) == 0 and int(out["plans"][0, 0]) == -1, name
            continue
        assert int(out["status"][0]) == native.MP_OK and int(out["plan_len"][0]) == 1, name
        assert int(order[out["plans"][0, 0]]) == int(case["plan"][0]) == int(order[out["best_challenger"][0, 0]]), name
        assert int(out["episodes_run"][0]) == int(case["episodes_run"]), name
        assert int(out["env_steps"][0]) == int(case["episodes_run"]) * int(case["horizon"]), name
        tree = ctx.gape_stoch_tree(0)
        chance = tree["kind"] == 1
        tree["action"] = np.where(chance, order[np.clip(tree["action"], 0, len(order) - 1)], tree["action"]).astype(np.int32)
        worst = max(worst, assert_tree(tree, golden_tree(case), float(case["gamma"]), name))
        # a decision node's state is its key (-1 for a placeholder), a chance node's its parent's
        dec = ~chance
        assert np.array_equal(tree["state"][dec][1:], np.maximum(tree["action"][dec][1:], -1)), name
        assert np.array_equal(tree["state"][chance], tree["state"][tree["parent"][chance]]), name
        # the root's arms as the call reports them: the tree's depth-0 chance nodes, by column
        arms = np.flatnonzero(chance & (tree["parent"] == 0))
        cols = column[tree["action"][arms]]
        assert np.array_equal(out["child_count"][0, cols], tree["count"][arms]), name
        assert np.array_equal(out["child_upper"][0, cols], tree["vu"][arms]), name
        assert np.array_equal(out["child_lower"][0, cols], tree["vl"][arms]), name
        assert (np.delete(out["child_count"][0], cols) == -1).all(), name
        planned += 1
    print("golden cases: max |device - reference| over mu_* and value_* =", worst)
    assert planned == 11


def test_every_golden_case_through_the_agent(z):
    from rl_agents_amd.agents.tree_search.mdp_gape import PLACEHOLDERS_MESSAGE, ChanceNode
    planned = 0
    for name in names(z):
        case = golden_case(z, name)
        env, agent = case_agent(case)
        if str(case["error"]):
            with pytest.raises(ValueError) as raised:
                agent.plan(int(case["s0"]))
            assert str(raised.value)[:20] == str(case["message"])[:20], name
            assert name != "placeholders" or str(raised.value) == str(case["message"]) == PLACEHOLDERS_MESSAGE
            # the draws and steps made before the reference raised
            assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
            assert agent.planner.env_steps == int(case["env_steps"]), name
            continue
        assert agent.plan(int(case["s0"])) == case["plan"].tolist(), name
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
        assert agent.planner.env_steps == int(case["env_steps"]), name
        assert agent.planner.budget_used == int(case["episodes_run"]) * int(case["horizon"]), name
        assert agent.planner.get_plan() == case["plan"].tolist(), name
        # the linked tree, listed as the golden file lists the reference's: dict order, placeholder keys as strings
        root = agent.planner.root
        nodes, parents, keys = [root], [-1], [-1]
        i = 0
        while i < len(nodes):
            for k, c in nodes[i].children.items():
                nodes.append(c)
                parents.append(i)
                keys.append(-1 - int(k[len("placeholder_"):]) if isinstance(k, str) and k.startswith("placeholder_") else int(k))
            i += 1
        dec = [not isinstance(n, ChanceNode) for n in nodes]
        tree = dict(parent=np.asarray(parents), kind=np.asarray([0 if d else 1 for d in dec]), action=np.asarray(keys),
                    depth=np.asarray([n.depth for n in nodes]), count=np.asarray([n.count for n in nodes]),
                    done=np.asarray([int(n.done) if d else 0 for n, d in zip(nodes, dec)]),
                    cum=np.asarray([n.cumulative_reward if d else 0.0 for n, d in zip(nodes, dec)]),
                    mu_ucb=np.asarray([n.mu_ucb if d else 0.0 for n, d in zip(nodes, dec)]),
                    mu_lcb=np.asarray([n.mu_lcb if d else 0.0 for n, d in zip(nodes, dec)]),
                    vu=np.asarray([n.value_upper for n in nodes]), vl=np.asarray([n.value_lower for n in nodes]))
        assert_tree(tree, golden_tree(case), float(case["gamma"]), name)
        assert root.selection_rule() == int(case["plan"][0]), name
        visits = agent.planner.get_visits()
        assert sum(visits.values()) == int(case["env_steps"]) and "None" not in visits, name
        planned += 1
    assert planned == 11


SMALL = generators.random_sparse(9, 3, 2, seed=121)
SMALL_CFG = dict(horizon=3, episodes=20, gamma=0.8, accuracy=2.0, max_next_states_count=2)   # (some plans stop early, some run out)


def small_env(s0=0):
    env = FiniteMDPEnv(dict(mode="sparse", transition=np.asarray(SMALL["transition"]).tolist(), next=np.asarray(SMALL["next"]).tolist(),
                            reward=np.asarray(SMALL["reward"]).tolist(), terminal=np.asarray(SMALL["terminal"]).astype(int).tolist(),
                            state=int(s0)))
    env.reset()
    return env


@pytest.mark.parametrize("n", [1, 2, 65])
def test_a_batch_equals_its_single_root_calls(n):
    env = small_env()
    agent = agent_factory(env, dict(SMALL_CFG, __class__=STOCH_AGENT))
    agent.seed(7)
    roots = (np.arange(n) * 5 % 9).astype(np.int32)
    rng = agent.planner.batch_rng_states(n)
    assert len({r.tobytes() for r in rng}) == n
    rng0 = rng.copy()
    out = agent.planner.plan_batch(env, roots, rng_states=rng)
    ctx = agent.planner.models.ctx
    assert_form(ctx, "gape_stoch_sparse")
    trees = {i: ctx.gape_stoch_tree(i) for i in (0, n - 1)}
    for i in range(n):
        one = rng0[i:i + 1].copy()
        single = agent.planner.plan_batch(env, roots[i:i + 1], rng_states=one)
        for k in RESULTS:
            assert np.array_equal(out[k][i], single[k][0]), (i, k)
        assert np.array_equal(rng[i], one[0]), i
        if i in trees:
            tree = ctx.gape_stoch_tree(0)
            assert all(np.array_equal(tree[k], trees[i][k]) for k in tree), i


def test_one_next_state_on_a_table_equals_mp_gape_plan_bit_for_bit(z):
    """K = 1 on a deterministic table: 1.0 * u == u and the clone's generator is never made, so every output and every exported
    field is mp_gape_plan's."""
    for name, n in (("det_k1", 1), ("finite_det_k2", 5)):
        case = dict(golden_case(z, name), max_next_states_count=1)
        env, agent = case_agent(case)
        agent.seed(5)
        planner = agent.planner
        ctx, model = planner.models.ctx, planner.model_for(env)
        roots = (int(case["s0"]) + np.arange(n)) % case["mdp/reward"].shape[0]
        rng_a = planner.batch_rng_states(n) if n > 1 else case["rng_before"].reshape(1, 6).copy()
        rng_b = rng_a.copy()
        args = (float(case["gamma"]), float(case["accuracy"]), str(case["continuation"]) == "uniform", model.A, None,
                planner.thresholds())
        new = ctx.gape_plan_stochastic(model, roots, int(case["episodes"]), int(case["horizon"]), 1, *args,
                                       planner.transition_thresholds(), planner._value_init, rng_a)
        assert_form(ctx, "gape_stoch_table")
        new_trees = [ctx.gape_stoch_tree(i) for i in range(n)]
        with pytest.raises(native.NativeError, match="no tree of mp_gape_plan"):
            ctx.gape_tree(0)
        old = ctx.gape_plan(model, roots, int(case["episodes"]), int(case["horizon"]), *args, planner._value_init, rng_b)
        assert_form(ctx, "gape_global")
        with pytest.raises(native.NativeError, match="no tree of mp_gape_plan_stochastic"):
            ctx.gape_stoch_tree(0)
        assert np.array_equal(rng_a, rng_b), name
        for k in RESULTS:
            assert np.array_equal(new[k], old[k]), (name, k)
        assert (new["status"] == native.MP_OK).all(), name
        for i in range(n):
            old_tree = ctx.gape_tree(i)
            bfs = dict(gr.as_bfs(old_tree))
            for k in bfs:
                assert np.array_equal(new_trees[i][k], bfs[k]), (name, i, k)      # bits: no tolerance


def test_refusals():
    env = small_env()
    agent = agent_factory(env, dict(SMALL_CFG, __class__=STOCH_AGENT))
    agent.seed(9)
    planner = agent.planner
    ctx, model = planner.models.ctx, planner.model_for(env)
    thr, tthr, vin = planner.thresholds(), planner.transition_thresholds(), planner._value_init

    def call(count=2, gamma=0.8, accuracy=1.0, thr=thr, tthr=tthr, vin=vin, model=model):
        rng = planner.batch_rng_states(1)
        return ctx.gape_plan_stochastic(model, [0], 20, 3, count, gamma, accuracy, True, 3, None, thr, tthr, vin, rng)

    assert int(call()["status"][0]) == native.MP_OK
    for count in (0, 33, -1):
        with pytest.raises(native.NativeError, match="1..32"):
            call(count=count)
    bad = lambda table, i, v: np.concatenate([table[:i], [v], table[i + 1:]])  # noqa: E731
    for kwargs, match in ((dict(thr=bad(thr, 3, np.nan)), "threshold of count 4"), (dict(tthr=bad(tthr, 21, np.inf)), "transition threshold of count 22"),
                          (dict(vin=bad(vin, 1, np.nan)), "initial value of depth 1"), (dict(gamma=np.nan), "gamma"),
                          (dict(accuracy=np.inf), "accuracy")):
        with pytest.raises(native.NativeError, match=match):
            call(**kwargs)
    # the trees of one planner are not the other's
    call()
    with pytest.raises(native.NativeError, match="no tree of mp_gape_plan on this ctx"):
        ctx.gape_tree(0)
    # more placeholders than a chance node ever needs: the plan is that of any K >= the next states there are
    a, b = call(count=2), call(count=32)
    assert int(b["status"][0]) == native.MP_OK and int(a["plans"][0, 0]) >= 0
    # the old agent still refuses this env
    with pytest.raises(TypeError, match="deterministic"):
        agent_factory(env, {"__class__": GAPE_AGENT, "budget": 50}).planner.plan_batch(env, [0])
