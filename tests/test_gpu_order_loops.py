"""The loops that run many agents at once -- PerEpisodeEvaluation (every kind), BatchedEvaluation (host-stepped and
device-resident) and the sharded planner in a world of one -- on environments whose listing order is NOT its own inverse and
no adjacent swap (tests/order_cases.py: (2, 0, 1), (2, 0, 4, 1, 3) and an 8-action permutation).  Every other GPU test sends
highway's (1, 0, 2, 3, 4) through these loops: a place that applies ``order[a]`` where the inverse was meant passes there, and
so does a row summed in device column order.

Everything is compared exactly: actions (environment ids), generator records, planner env steps, and -- for the prior kinds --
the policy rows the loop uploads, by bits."""
import os

import numpy as np
import pytest

from rl_agents_amd import native
from tests import order_cases as oc

pytestmark = pytest.mark.gpu

E, T_STEPS = 4, 3
HERE = os.path.dirname(os.path.abspath(__file__))
VI = "<class 'rl_agents_amd.agents.dynamic_programming.value_iteration.ValueIterationAgent'>"
UCT = "<class 'rl_agents_amd.agents.tree_search.mcts.MCTSAgent'>"
OPD = "<class 'rl_agents_amd.agents.tree_search.deterministic.DeterministicPlannerAgent'>"


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(HERE, "golden", "per_episode_order.npz"))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).tobytes()


def _record_uploads(ev):
    """The [N, S, A] rows the loop uploads, one entry per lock-step."""
    uploads, real = [], ev._prior_tables

    def recording(live):
        tables = real(live)
        uploads.append((list(live), np.array(tables)))
        return tables
    ev._prior_tables = recording
    return uploads


# ------------------------------------------------------------------------------------------ against the unmodified reference
def _golden_envs(z, name):
    from rl_agents_amd.envs import OrderedMaskedScheduledTableEnv
    order = [int(a) for a in z[name + "/order"]]
    oc.assert_general_order(order)
    envs = []
    for e in range(E):
        tables = [dict(mode="deterministic", transition=z[name + "/transition"][e, t], reward=z[name + "/reward"][e, t],
                       terminal=z[name + "/terminal"][e, t]) for t in range(T_STEPS)]
        tables[0].update(available=z[name + "/available"].astype(int), listing_order=order)
        envs.append(OrderedMaskedScheduledTableEnv(tables, state=int(z[name + "/s0"][e])))
    return envs


def _golden_agent(z, name, kind, env):
    from rl_agents_amd.agents.tree_search.deterministic import DeterministicPlannerAgent
    from rl_agents_amd.agents.tree_search.mcts import MCTSAgent
    from rl_agents_amd.agents.tree_search.mcts_with_prior import MCTSWithPriorPolicyAgent
    base = "{}/{}/".format(name, kind)
    cfg = dict(budget=int(z[base + "budget"]), gamma=float(z[base + "gamma"]))
    if kind == "opd":
        return DeterministicPlannerAgent(env, cfg)
    cfg["temperature"] = float(z[base + "temperature"])
    if kind == "subtree":
        agent = MCTSAgent(env, dict(cfg, step_strategy="subtree"))
    elif kind == "uct":
        agent = MCTSAgent(env, dict(cfg, prior_policy={"type": "preference", "action": 2, "ratio": 3},
                                    rollout_policy={"type": "random_available"}))
    else:
        agent = MCTSWithPriorPolicyAgent(env, dict(cfg, prior_agent={
            "__class__": VI, "gamma": float(z["prior/gamma"]), "iterations": int(z["prior/iterations"]),
            "temperature": float(z["prior/temperature"])}))
    assert agent.planner.config["episodes"] == int(z[base + "episodes"]) and agent.planner.config["horizon"] == int(z[base + "horizon"])
    return agent


@pytest.mark.parametrize("kind", ["prior", "uct", "opd", "subtree"])
@pytest.mark.parametrize("name", ["a3", "a5"])
def test_golden_per_episode_order(z, name, kind):
    """tests/golden/per_episode_order.npz: four episodes of the UNMODIFIED reference, one agent object each, on restricted action
    sets listed in an order that is not its own inverse, the table replaced before every step -- first actions, episode lengths,
    the generator of every episode and the planner's env steps from one batched launch per step; `prior`: the uploaded rows are
    the reference's own Boltzmann rows, restricted with its own formula, by bits; `subtree`: MCTS that keeps its subtrees, which on
    restricted action sets only the reference can vouch for (see the sequential test below)."""
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    envs = _golden_envs(z, name)
    ev = PerEpisodeEvaluation(envs, _golden_agent(z, name, kind, envs[0]), sim_seed=dict(prior=500, uct=600, opd=700, subtree=800)[kind],
                              max_steps=T_STEPS)
    uploads = _record_uploads(ev)
    out = ev.run()
    order, available = [int(a) for a in z[name + "/order"]], z[name + "/available"].astype(bool)
    base, total = "{}/{}".format(name, kind), 0
    for e in range(E):
        p = "{}/e{}".format(base, e)
        states = z[p + "/states"]
        n_steps = len(states)
        assert int(out["lengths"][e]) == n_steps
        for t in range(n_steps):
            assert int(out["actions"][e, t]) == int(z[p + "/plan"][t, 0]), (p, t)
            # (a kept node keeps the children it was given in the state of the table it was expanded on: with kept subtrees the
            # reference's own action need not be listed in the state the new table puts the episode in)
            assert kind == "subtree" or available[int(states[t]), int(out["actions"][e, t])], (p, t)
            if kind == "prior":
                live, tables = uploads[t]
                assert e in live
                assert _bits(tables[e]) == _bits(oc.reference_rows(z[p + "/prior_table"][t], order, available)), (p, t)
        total += int(z[p + "/env_steps_total"][n_steps - 1])
        np.testing.assert_array_equal(ev.rng[e], z[p + "/rng_after"][n_steps - 1], err_msg=p)
    assert out["planner_env_steps"] == total
    assert len(uploads) == (T_STEPS if kind == "prior" else 0) and ev.subtree == (kind == "subtree")
    ev.close()


# ------------------------------------------------------------------------------------------ against N sequential agent loops
def _sequential(envs, make_agent, sim_seed, max_steps):
    """N separate (environment, agent) loops, one agent object per episode as the reference runs them (the pattern of
    tests/test_gpu_per_episode_eval.py) -> actions, returns, the agents."""
    acts = np.full((len(envs), max_steps), -1, np.int32)
    returns, agents = np.zeros(len(envs)), []
    for i, env in enumerate(envs):
        obs, _ = env.reset()
        agent = make_agent(env)
        agents.append(agent)
        if hasattr(agent, "seed"):
            agent.seed(sim_seed + i)
        for t in range(max_steps):
            a = int(agent.act(obs))
            obs, r, term, trunc, _ = env.step(a)
            acts[i, t] = a
            returns[i] += r
            if term or trunc:
                break
    return acts, returns, agents


def _kinds():
    from rl_agents_amd.agents.dynamic_programming.value_iteration import ValueIterationAgent
    from rl_agents_amd.agents.tree_search.brue import BRUEAgent
    from rl_agents_amd.agents.tree_search.deterministic import DeterministicPlannerAgent
    from rl_agents_amd.agents.tree_search.mcts import MCTSAgent
    from rl_agents_amd.agents.tree_search.mcts_with_prior import MCTSWithPriorPolicyAgent
    from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapEAgent
    from rl_agents_amd.agents.tree_search.olop import OLOPAgent
    from rl_agents_amd.agents.tree_search.sparse_sampling import SparseSamplingAgent
    prior = dict(gamma=0.9, iterations=100, temperature=0.3)
    # kind -> (agent class, config, kind= of the loop, environments that convert on request)
    return dict(
        vi=(ValueIterationAgent, dict(gamma=0.95, iterations=100), None, True),
        uct=(MCTSAgent, dict(budget=150, gamma=0.8, prior_policy={"type": "preference", "action": 2, "ratio": 3},
                             rollout_policy={"type": "random_available"}), None, False),
        uct_random=(MCTSAgent, dict(budget=150, gamma=0.8, prior_policy={"type": "random"}, rollout_policy={"type": "random"}),
                    None, False),
        uct_subtree=(MCTSAgent, dict(budget=150, gamma=0.8, step_strategy="subtree"), None, False),
        uct_vi_prior=(MCTSWithPriorPolicyAgent, dict(budget=120, gamma=0.8, temperature=6.0,
                                                     prior_agent=dict(prior, __class__=VI)), None, True),
        uct_other_prior=(MCTSWithPriorPolicyAgent, dict(budget=120, gamma=0.8, temperature=6.0,
                                                        prior_agent=dict(prior, __class__=oc.TABULATED_VI)), None, True),
        opd=(DeterministicPlannerAgent, dict(budget=120, gamma=0.8), None, False),
        olop=(OLOPAgent, dict(budget=150, gamma=0.8, upper_bound={"type": "kullback-leibler"}, continuation_type="uniform"),
              None, False),
        brue=(BRUEAgent, dict(budget=100, gamma=0.8), None, False),
        gape=(MDPGapEAgent, dict(horizon=4, episodes=12, gamma=0.8, accuracy=0.1,
                                 upper_bound=dict(type="kullback-leibler", threshold="1*np.log(time)")), "gape", False),
        ss=(SparseSamplingAgent, dict(horizon=3, C=2, gamma=0.8), "ss", False),
    )


CASES = [(kind, "a5") for kind in ("vi", "uct", "uct_random", "uct_vi_prior", "uct_other_prior", "opd", "olop", "brue", "gape", "ss")]
# kept subtrees: this package's SINGLE agent looks a kept node's priors and child set up by the state the descent is in, which
# is exact only where they do not depend on the state (tests/test_gpu_per_episode_subtree.py compares `plain/uct` alone) -- so
# the sequential agents can speak for the loop on the re-ordered fixture that lists every action; the restricted fixtures are
# compared with the reference itself (test_golden_per_episode_order[*-subtree])
CASES += [("uct_subtree", "a8_full")]
CASES += [(kind, name) for name in ("a3", "a8", "a8_full") for kind in ("uct", "uct_vi_prior", "uct_other_prior", "opd")]


@pytest.mark.parametrize("kind,name", CASES)
def test_changing_ordered_batch_equals_sequential_agents(kind, name):
    """Eight environments that list restricted action sets in an order that is not its own inverse, each with a table replaced
    before every step: the batch == eight sequential (environment, agent) loops -- actions, returns, every episode's generator,
    the planners' env steps; the prior kinds: the rows uploaded at every step == each sequential agent's own table, by bits."""
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    oc.assert_general_order(oc.ORDERS[name])
    n, steps = 8, 3
    cls, cfg, loop_kind, converted = _kinds()[kind]

    def envs():
        made = [oc.scheduled_env(name, i, steps, seed=1000) for i in range(n)]
        return [oc.ConvertedOrderedEnv(env) for env in made] if converted else made
    batch_envs = envs()
    ev = PerEpisodeEvaluation(batch_envs, cls(batch_envs[0], dict(cfg)), sim_seed=7, max_steps=steps, kind=loop_kind)
    assert ev.kind == (loop_kind or ("uct" if kind.startswith("uct") else kind))
    uploads = _record_uploads(ev)
    out = ev.run()
    with_prior = kind.endswith("_prior")
    tables = []                                             # [episode][step] of the sequential agents

    def make_agent(env):
        agent = cls(env, dict(cfg))
        if with_prior:
            rows, source = [], agent.planner.policy_source
            tables.append(rows)

            def recording(state, model):
                got = source(state, model)
                rows.append(np.array(got[0]))
                return got
            agent.planner.policy_source = recording
        return agent
    acts, returns, agents = _sequential(envs(), make_agent, 7, steps)
    np.testing.assert_array_equal(out["actions"], acts)
    assert np.array_equal(out["returns"], returns)
    assert (out["actions"][:, 0] >= 0).all() and out["lengths"].max() == steps
    if kind != "vi":
        for i, agent in enumerate(agents):
            np.testing.assert_array_equal(ev.rng[i], native.rng_state_from_generator(agent.planner.np_random), err_msg=str(i))
        assert out["planner_env_steps"] == sum(int(agent.planner.env_steps) for agent in agents)
    if with_prior:
        assert len(uploads) == steps
        for t, (live, batch_tables) in enumerate(uploads):
            assert live == [i for i in range(n) if out["lengths"][i] > t]
            for i in live:
                assert _bits(batch_tables[i]) == _bits(tables[i][t]), (i, t)
    if kind == "uct_random":
        assert ev.model.action_order is None            # (policy type `random` lists np.arange(n): _extract drops the order)
    elif kind not in ("vi", "brue"):
        assert tuple(int(a) for a in ev.model.action_order) == oc.ORDERS[name]
    ev.close()


# ------------------------------------------------------------------------------------------ the robust planner
def _robust_config(name):
    other = oc.table(name, 0, 0, seed=77)
    args = dict(mode="deterministic", transition=other["transition"].tolist(), reward=other["reward"].tolist(),
                terminal=np.asarray(other["terminal"]).astype(int).tolist())
    return dict(budget=120, gamma=0.8, models=[[], [{"method": "copy_with_config", "args": args}]])


def test_ordered_joint_union_listed_ascending_equals_sequential_robust_agents():
    """JointEnv lists list(set().union(...)) of what its models list: the models' own (2, 0, 4, 1, 3) is lost in the set, and
    for five small action ids the set comes out ascending -- the loop plans, and equals six sequential robust agents."""
    from rl_agents_amd.agents.robust.robust import DiscreteRobustPlannerAgent
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    name, n, steps = "a5", 6, 3
    oc.assert_general_order(oc.ORDERS[name])
    cfg = _robust_config(name)

    def envs():
        return [oc.scheduled_env(name, i, steps, seed=2000) for i in range(n)]
    batch_envs = envs()
    assert batch_envs[0].get_available_actions() != sorted(batch_envs[0].get_available_actions())
    ev = PerEpisodeEvaluation(batch_envs, DiscreteRobustPlannerAgent(batch_envs[0], dict(cfg)), sim_seed=7, max_steps=steps)
    assert ev.kind == "ropd"
    out = ev.run()
    acts, returns, agents = _sequential(envs(), lambda env: DiscreteRobustPlannerAgent(env, dict(cfg)), 7, steps)
    np.testing.assert_array_equal(out["actions"], acts)
    assert np.array_equal(out["returns"], returns)
    for i, agent in enumerate(agents):
        np.testing.assert_array_equal(ev.rng[i], native.rng_state_from_generator(agent.planner.np_random), err_msg=str(i))
    assert out["planner_env_steps"] == sum(int(agent.planner.env_steps) for agent in agents)
    assert out["lengths"].max() == steps
    ev.close()


def test_ordered_joint_union_not_listed_ascending_is_refused():
    """A union the set does NOT list ascending: ten actions listed (8, 1, 3, 0, ...), a start state that lists 8 and 1 only --
    CPython iterates {8, 1} as 8, 1 (8 lands in slot 0 of the set's eight) -- and the device would expand 1 before 8."""
    from rl_agents_amd.agents.robust.robust import DiscreteRobustPlannerAgent
    from rl_agents_amd.envs import OrderedMaskedScheduledTableEnv, generators
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    order = (8, 1, 3, 0, 2, 4, 5, 6, 7, 9)
    oc.assert_general_order(order)
    assert list(set().union([8, 1])) == [8, 1]
    available = np.ones((12, 10), dtype=bool)
    available[0] = False
    available[0, [8, 1]] = True

    def env(i):
        tabs = [dict(generators.random_deterministic(12, 10, seed=300 + 10 * i + t)) for t in range(2)]
        tabs[0].update(available=available.astype(int), listing_order=list(order))
        return OrderedMaskedScheduledTableEnv(tabs, state=0)
    envs = [env(i) for i in range(2)]
    other = generators.random_deterministic(12, 10, seed=5)
    args = dict(mode="deterministic", transition=other["transition"].tolist(), reward=other["reward"].tolist(),
                terminal=np.asarray(other["terminal"]).astype(int).tolist())
    cfg = dict(budget=60, gamma=0.8, models=[[], [{"method": "copy_with_config", "args": args}]])
    ev = PerEpisodeEvaluation(envs, DiscreteRobustPlannerAgent(envs[0], cfg), sim_seed=7, max_steps=2)
    with pytest.raises(NotImplementedError, match=r"ascending order, got \[8, 1\]"):
        ev.run()
    ev.close()


# ------------------------------------------------------------------------------------------ BatchedEvaluation, static table
def _replay_is_listed(name, env, starts, actions):
    """Every logged action is an ENVIRONMENT id: listed by the environment in the state the episode was in."""
    available, transition = oc.available_of(name), np.asarray(env.mdp.transition)
    for i, s in enumerate(starts):
        for a in actions[i]:
            if a < 0:
                break
            assert available[int(s), int(a)], (i, int(s), int(a))
            s = transition[int(s), int(a)]


@pytest.mark.parametrize("name", ["a5", "a8"])
@pytest.mark.parametrize("kind", ["uct", "opd"])
def test_device_resident_loop_equals_host_stepped_loop_and_sequential_agents(kind, name):
    """One static table, restricted action sets listed in an order that is not its own inverse: the device-resident loop == the
    host-stepped loop == twelve sequential agents; the logged actions are the environment's ids."""
    from rl_agents_amd.agents.common.factory import agent_factory
    from rl_agents_amd.trainer.batched_evaluation import BatchedEvaluation
    oc.assert_general_order(oc.ORDERS[name])
    cfg = dict(__class__=UCT, budget=150, gamma=0.8) if kind == "uct" else dict(__class__=OPD, budget=120, gamma=0.8)
    n, steps = 12, 4
    terminal = np.asarray(oc.static_env(name).mdp.terminal)
    starts = np.flatnonzero(~terminal)[(np.arange(n) * 5) % int((~terminal).sum())].astype(np.int32)
    runs = []
    for resident in (False, True):
        env = oc.static_env(name)
        ev = BatchedEvaluation(env, agent_factory(env, dict(cfg)), num_episodes=n, sim_seed=40, max_steps=steps,
                               device_resident=resident, check_every=2)
        runs.append(ev.run(initial_states=starts))
        assert runs[-1]["device_resident"] is resident
    acts = np.full((n, steps), -1, np.int32)
    returns, env_steps = np.zeros(n), 0
    for i in range(n):
        env = oc.static_env(name, state=starts[i])
        agent = agent_factory(env, dict(cfg))
        agent.seed(40 + i)
        obs = int(env.mdp.state)
        for t in range(steps):
            a = int(agent.act(obs))
            obs, r, term, trunc, _ = env.step(a)
            acts[i, t] = a
            returns[i] += r
            if term or trunc:
                break
        env_steps += int(agent.planner.env_steps)
    for run in runs:
        np.testing.assert_array_equal(run["actions"], acts)
        np.testing.assert_array_equal(run["lengths"], (acts >= 0).sum(axis=1))
        assert np.array_equal(run["returns"], returns)
        assert run["planner_env_steps"] == env_steps
        _replay_is_listed(name, oc.static_env(name), starts, run["actions"])
    assert np.array_equal(runs[0]["discounted_returns"], runs[1]["discounted_returns"])


# ------------------------------------------------------------------------------------------ the sharded planner, world of one
@pytest.mark.parametrize("kind", ["uct", "opd"])
def test_sharded_planner_in_a_world_of_one_returns_environment_ids(kind):
    """No process group: plan_batch_sharded, plan_batch_sharded_device and two consecutive ShardedDevicePlan.plan() calls on an
    ordered model == the single agent's plan_batch on the same roots and generator records; the plans are environment ids."""
    import torch
    from rl_agents_amd.agents.common.factory import agent_factory
    from rl_agents_amd.distributed import ShardedDevicePlan, plan_batch_sharded, plan_batch_sharded_device
    name = "a5"
    order = oc.ORDERS[name]
    oc.assert_general_order(order)
    cfg = dict(__class__=UCT, budget=150, gamma=0.8) if kind == "uct" else dict(__class__=OPD, budget=120, gamma=0.8)
    available, terminal = oc.available_of(name), np.asarray(oc.static_env(name).mdp.terminal)
    roots = np.tile(np.flatnonzero(~terminal), 5)[:70].astype(np.int32)          # more than a wavefront, ragged
    n = len(roots)

    def agent():
        env = oc.static_env(name)
        made = agent_factory(env, dict(cfg))
        made.seed(77)
        return made
    single = agent()
    rng = single.planner.batch_rng_states(n)
    want = single.planner.plan_batch(single.planning_env(), roots, None, rng_states=rng)
    assert tuple(int(a) for a in single.planner.action_order(single.planner.model_for(single.planning_env()))) == order
    assert available[roots, want["plans"][:, 0]].all(), "the single agent's first actions are listed in their roots"
    labels = oc.inverse_of(order)[want["plans"][:, 0]]
    assert not available[roots, labels].all(), "the case cannot tell device labels from environment ids"
    host = plan_batch_sharded(agent(), roots)
    for k in ("plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(host[k], want[k], err_msg=k)
    width = want["plans"].shape[1]
    d_roots = torch.from_numpy(roots).cuda()
    out = plan_batch_sharded_device(agent(), d_roots, max_plan_len=width)
    np.testing.assert_array_equal(out["plans"].cpu().numpy(), want["plans"])
    np.testing.assert_array_equal(out["env_steps"].cpu().numpy(), want["env_steps"])
    # two consecutive plans: the generator records stay resident and continue as the single agent's do
    again = single.planner.plan_batch(single.planning_env(), roots[::-1].copy(), None, rng_states=rng)
    sp = ShardedDevicePlan(agent(), n, max_plan_len=width, payload="full")
    first = sp.wait(sp.plan(d_roots))
    np.testing.assert_array_equal(first["plans"].cpu().numpy(), want["plans"])
    second = sp.wait(sp.plan(torch.from_numpy(roots[::-1].copy()).cuda()))
    np.testing.assert_array_equal(second["plans"].cpu().numpy(), again["plans"])
    np.testing.assert_array_equal(second["env_steps"].cpu().numpy(), again["env_steps"])
    np.testing.assert_array_equal(sp.d_rng.cpu().numpy().view(np.uint64), rng)
    assert not second["status"].cpu().numpy().any()
