"""PerEpisodeEvaluation with OLOPAgent and BRUEAgent: N environments that each own a finite MDP which changes at every step, one
batched launch per step on one MDP per root (mp_olop_plan_models / mp_brue_plan_models) -- equal to the unmodified reference's
per-episode agents (tests/golden/per_episode_olop_brue.npz) and to N sequential (environment, agent) loops of this package's
single agents.  Everything is compared exactly, but OLOP's root value_upper: 1e-12, the tolerance for the device's log in the
KL bound's Newton step."""
import os

import numpy as np
import pytest

from rl_agents_amd import native

pytestmark = pytest.mark.gpu

E, T_STEPS = 6, 3
HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = dict(olop={"budget": 150, "gamma": 0.8, "upper_bound": {"type": "kullback-leibler"}, "continuation_type": "uniform"},
               brue={"budget": 120, "gamma": 0.8})


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(HERE, "golden", "per_episode_olop_brue.npz"))


def agent_class(kind):
    from rl_agents_amd.agents.tree_search.brue import BRUEAgent
    from rl_agents_amd.agents.tree_search.olop import OLOPAgent
    return OLOPAgent if kind == "olop" else BRUEAgent


def _scheduled_envs(z):
    from rl_agents_amd.envs import ScheduledTableEnv
    envs = []
    for e in range(E):
        tables = [dict(mode="deterministic", transition=z["transition"][e, t], reward=z["reward"][e, t],
                       terminal=z["terminal"][e, t]) for t in range(T_STEPS)]
        envs.append(ScheduledTableEnv(tables, state=int(z["s0"][e])))
    return envs


@pytest.mark.parametrize("kind", ["olop", "brue"])
def test_golden_per_episode_evaluation(z, kind):
    """Six episodes of the reference, each with its own agent object and a table replaced before every step: the first action
    of every step, the generator of every episode and the planner's env steps, from one batched launch per step."""
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    envs = _scheduled_envs(z)
    agent = agent_class(kind)(envs[0], dict(CONFIGS[kind]))
    pc = agent.planner.config
    assert pc["horizon"] == int(z[kind + "/horizon"]) and (kind == "brue" or pc["episodes"] == int(z["olop/episodes"]))
    ev = PerEpisodeEvaluation(envs, agent, sim_seed=100, max_steps=T_STEPS)
    assert ev.kind == kind
    out = ev.run()
    assert ev.ctx.last_kernel_variant().startswith(kind + "_each_")
    n_steps = [int(z["{}/e{}/n_steps".format(kind, e)]) for e in range(E)]     # (the reference drives some episodes into a
    assert min(n_steps) >= 2 and max(n_steps) == T_STEPS                        # terminal state with its second action)
    for e in range(E):
        assert int(out["lengths"][e]) == n_steps[e]
        for t in range(n_steps[e]):
            p = "{}/e{}/t{}".format(kind, e, t)
            assert int(out["actions"][e, t]) == int(z[p + "/plan"][0]), p
        np.testing.assert_array_equal(ev.rng[e], z["{}/e{}/t{}/rng_after".format(kind, e, n_steps[e] - 1)])
    total = sum(int(z["{}/e{}/t{}/env_steps_total".format(kind, e, n_steps[e] - 1)]) for e in range(E))
    assert out["planner_env_steps"] == total
    # every table changed at every step: the table of every step an episode lived to see was sent exactly once (E * T_STEPS
    # where no episode ends early)
    assert out["uploads"] == sum(n_steps)
    ev.close()


def test_golden_steps_through_the_entry_point(z):
    """The fixture's steps planned directly with olop_plan(..., model_index=...): the whole plan of every step exactly, the
    generator records exactly, and the reference's root value_upper within 1e-12."""
    from rl_agents_amd.agents.tree_search.olop import OLOP
    ctx = native.Context(0)
    episodes, horizon, gamma = int(z["olop/episodes"]), int(z["olop/horizon"]), float(z["olop/gamma"])
    thr = np.full(episodes, float(4 * np.log(episodes)))          # "4*np.log(time)", time = the number of episodes
    rng = np.stack([z["olop/e{}/rng_before".format(e)] for e in range(E)])
    model = None
    for t in range(T_STEPS):
        tr, rw, term = z["transition"][:, t], z["reward"][:, t], z["terminal"][:, t].astype(np.uint8)
        if model is None:
            model = ctx.load_table_batch(tr, rw, term)
        else:
            model.update_tables(0, tr, rw, term)
        live = np.array([e for e in range(E) if t < int(z["olop/e{}/n_steps".format(e)])], np.int32)
        states = np.array([z["olop/e{}/states".format(e)][t] for e in live], np.int32)
        live_rng = np.ascontiguousarray(rng[live])
        out = ctx.olop_plan(model, states, episodes, horizon, gamma, True, -1, thr, OLOP.value_upper_init(gamma, horizon),
                            live_rng, model_index=live)
        rng[live] = live_rng
        for k, e in enumerate(live):
            p = "olop/e{}/t{}".format(e, t)
            assert out["plans"][k, :out["plan_len"][k]].tolist() == z[p + "/plan"].tolist(), p
            np.testing.assert_array_equal(rng[e], z[p + "/rng_after"], err_msg=p)
            assert abs(out["root_value"][k] - float(z[p + "/root_value_upper"])) <= 1e-12, p
    model.close()


def _sequential(envs, make_agent, sim_seed, max_steps):
    """N separate (environment, agent) loops, one agent object per episode as the reference runs them."""
    acts = np.full((len(envs), max_steps), -1, np.int32)
    returns = np.zeros(len(envs))
    for i, env in enumerate(envs):
        obs, _ = env.reset()
        agent = make_agent(env)
        agent.seed(sim_seed + i)
        for t in range(max_steps):
            a = int(agent.act(obs))
            obs, r, term, trunc, _ = env.step(a)
            acts[i, t] = a
            returns[i] += r
            if term or trunc:
                break
    return acts, returns


def _highway_envs(n, seed0=500, lane=None):
    from rl_agents_amd.envs import ChangingHighwayEnv
    return [ChangingHighwayEnv(3, 4, 10, table_seed=seed0 + 20 * i, state=((i % 3) * 4 + (i % 4 if lane is None else lane)) * 10,
                               collision_rate=0.03 + 0.02 * (i % 4)) for i in range(n)]


@pytest.mark.parametrize("kind", ["olop", "brue"])
def test_changing_highway_batch_equals_sequential_agents(kind):
    """highway-env's surface (restricted action sets listed IDLE first, the restriction on the env object) with a table re-drawn
    after every step, 24 environments: batch == 24 sequential agent loops, action for action.  (Before these planners had their
    own kinds the loop ran the optimistic deterministic planner in their place.)"""
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    n, steps = 24, 6
    cls = agent_class(kind)
    cfg = dict(CONFIGS[kind], budget=150 if kind == "olop" else 100)
    batch_envs = _highway_envs(n)
    ev = PerEpisodeEvaluation(batch_envs, cls(batch_envs[0], dict(cfg)), sim_seed=7, max_steps=steps)
    out = ev.run()
    acts, returns = _sequential(_highway_envs(n), lambda env: cls(env, dict(cfg)), 7, steps)
    np.testing.assert_array_equal(out["actions"], acts)
    assert np.array_equal(out["returns"], returns)
    assert (out["actions"][:, 0] >= 0).all() and out["uploads"] >= n
    ev.close()


def test_zeros_continuation_without_action_0_raises_key_error():
    """OLOP's default continuation takes action 0 after an expansion (olop.py:89); in the leftmost lane the environment does
    not list LANE_LEFT = 0: KeyError(0) from the single agent and from the batch, whose generators have made their draws."""
    from rl_agents_amd.agents.tree_search.olop import OLOPAgent
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    cfg = {"budget": 100, "gamma": 0.8, "upper_bound": {"type": "kullback-leibler"}}
    env = _highway_envs(1, lane=0)[0]
    obs, _ = env.reset()
    single = OLOPAgent(env, dict(cfg))
    single.seed(7)
    with pytest.raises(KeyError):
        single.act(obs)
    envs = _highway_envs(4, lane=0)
    ev = PerEpisodeEvaluation(envs, OLOPAgent(envs[0], dict(cfg)), sim_seed=7, max_steps=3)
    with pytest.raises(KeyError):
        ev.run()
    before = native.seed_sequence_states((), 7, 4)
    assert all(not np.array_equal(ev.rng[i], before[i]) for i in range(4))
    np.testing.assert_array_equal(ev.rng[0], native.rng_state_from_generator(single.planner.np_random))
    ev.close()
