#!/usr/bin/env python3
"""Golden vectors for MDP-GapE WITH SEVERAL NEXT STATES PER CHANCE NODE on a BATCH OF EPISODES WITH THEIR OWN, PER-STEP-CHANGING
TABLES (tests/golden/per_episode_gape_stoch.npz).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_per_episode_gape_stoch.py      (build container only)

As make_golden_per_episode_gape.py: the same tables (``table(e, t)`` of make_golden_per_episode.py with the rewards clipped to
[1e-3, 1 - 1e-3]), the same start states and the seeds 100 + e, the UNMODIFIED reference ``MDPGapEAgent`` -- one object per
episode -- driven step by step through the stale-API adapters, none of which changes what it computes; here with
``max_next_states_count`` K > 1 and the ``StochObservers`` of make_golden_gape_stoch.py installed around every plan, which also
record every pair the transition bound compares.  On a deterministic table a chance node observes one next state, and its K - 1
placeholders left take mass in the KL solve: the plans differ from those of K = 1.

Two configs: "k2" (horizon 3, 20 episodes, K 2) and "k3" (horizon 4, 30 episodes, K 3), both gamma 0.8, accuracy 0 and the
threshold ``1*np.log(time)``.  The reference's own HighwayEnv/agents/BaiMCTSAgent/bai-olop.json (horizon 2, 100 episodes, K 2)
cannot be a fixture on these tables: it compares bounds 2.2e-16 apart (as it does at 40 episodes), which no device with another
``log`` can be held to, and MARGIN is not loosened for it.

The script REFUSES to write a file unless every plan's smallest margin exceeds MARGIN, an episode ends by its own actions before
the last step, and every plan made a tie draw.  Per step: the plan, the generator record before and after it, ``episodes_run``,
``env_steps`` of this plan, and the root's arms in creation order (action, count, lower, upper); for one plan of each config the
whole tree in the breadth-first layout of make_golden_gape_stoch.tree_listing.  Data only: inputs and outputs.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_gape_stoch import GAPE, MARGIN, StochObservers, tree_listing  # noqa: E402  (np.infty is aliased first)
from make_golden_olop import StaleApiEnv, StaleGenerator  # noqa: E402
from make_golden import agent_factory, np, rng_state  # noqa: E402
from make_golden_per_episode import E, L, T_STEPS, TT, V, install, table  # noqa: E402
from make_golden_per_episode_gape import TREE_AT, clipped  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "per_episode_gape_stoch.npz"))
LOG_TIME = {"type": "kullback-leibler", "threshold": "1*np.log(time)"}
CONFIGS = {
    "k2": dict(horizon=3, episodes=20, gamma=0.8, accuracy=0.0, max_next_states_count=2, upper_bound=LOG_TIME),
    "k3": dict(horizon=4, episodes=30, gamma=0.8, accuracy=0.0, max_next_states_count=3, upper_bound=LOG_TIME),
}


def run_episode(name, agent_cfg, e, start, tabs):
    """One reference agent, seeded 100 + e, on episode e's tables from state ``start`` -> (arrays, steps, margins, tie draws)."""
    store, margins, draws = {}, [], []
    cfg0 = dict(tabs[0])
    cfg0.pop("original_shape", None)
    cfg0["state"] = int(start)
    env = FiniteMDPEnv(cfg0)
    env.reset()
    agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=GAPE))
    agent.seed(100 + e)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    pc, ub = planner.config, planner.config["upper_bound"]
    for k in ("gamma", "horizon", "episodes", "accuracy", "confidence", "budget", "max_next_states_count"):
        store["{}/{}".format(name, k)] = np.asarray(pc[k])
    store["{}/continuation".format(name)] = np.asarray(pc["continuation_type"])
    store["{}/threshold".format(name)] = np.asarray(ub["threshold"])
    store["{}/transition_threshold".format(name)] = np.asarray(ub["transition_threshold"])
    states, n_steps = [], 0
    for t in range(T_STEPS):
        install(env, tabs[t])
        s = env.mdp.state
        states.append(s)
        p = "{}/e{}/t{}".format(name, e, t)
        planner.np_random = StaleGenerator(planner.np_random.bit_generator)
        store[p + "/rng_before"] = rng_state(planner.np_random)
        steps_before = len(planner.observations)
        obs = StochObservers()
        obs.install()
        try:
            plan = [int(a) for a in agent.plan(s)]
        finally:
            obs.remove()
        assert planner.budget_used % pc["horizon"] == 0
        arms = list(planner.root.children.items())
        store[p + "/plan"] = np.asarray(plan, np.int32)
        store[p + "/rng_after"] = rng_state(planner.np_random)
        store[p + "/episodes_run"] = np.asarray(planner.budget_used // pc["horizon"])
        store[p + "/env_steps"] = np.asarray(len(planner.observations) - steps_before)
        store[p + "/arm_action"] = np.asarray([int(a) for a, _ in arms], np.int32)
        store[p + "/arm_count"] = np.asarray([c.count for _, c in arms], np.int64)
        store[p + "/arm_lower"] = np.asarray([float(c.value_lower) for _, c in arms])
        store[p + "/arm_upper"] = np.asarray([float(c.value_upper) for _, c in arms])
        store[p + "/tie_draws"] = np.asarray(obs.tie_draws)
        store[p + "/margin"] = np.asarray(obs.smallest_margin())
        if (e, t) == TREE_AT:
            for k, v in tree_listing(planner.root).items():
                store[p + "/tree/" + k] = v
        margins.append(obs.smallest_margin())
        draws.append(obs.tie_draws)
        n_steps += 1
        _, _, term, trunc, _ = env.step(plan[0])
        if term or trunc:
            break
    store["{}/e{}/states".format(name, e)] = np.asarray(states, np.int64)
    store["{}/e{}/n_steps".format(name, e)] = np.asarray(n_steps)
    return store, n_steps, margins, draws


def main():
    store = {}
    tabs = [[clipped(table(e, t)) for t in range(T_STEPS)] for e in range(E + 1)]
    s0 = [((e % V) * L + (e % L)) * TT for e in range(E + 1)]          # time slice 0 of some (speed, lane)
    ended_early = False
    for name, agent_cfg in CONFIGS.items():
        lengths, margins, draws = [], [], []
        for e in range(E + 1):
            arrays, n_steps, m, d = run_episode(name, agent_cfg, e, s0[e], tabs[e])
            store.update(arrays)
            lengths.append(n_steps)
            margins += m
            draws += d
        print("{:4s} steps {} smallest margin {:.3g} tie draws {}..{}".format(name, lengths, min(margins), min(draws), max(draws)))
        assert min(margins) > MARGIN, "{}: two compared values are {} apart".format(name, min(margins))
        assert min(draws) >= 1, "{}: a plan without a tie draw".format(name)
        ended_early |= min(lengths) < T_STEPS
        store["{}/margin".format(name)] = np.asarray(min(margins))
    assert ended_early, "no episode of any config ends by its own actions before the last step"
    store["configs"] = np.asarray(list(CONFIGS))
    store["transition"] = np.stack([np.stack([c["transition"] for c in row]) for row in tabs]).astype(np.int64)   # [E + 1,T,S,A]
    store["reward"] = np.stack([np.stack([c["reward"] for c in row]) for row in tabs]).astype(np.float64)
    store["terminal"] = np.stack([np.stack([c["terminal"] for c in row]) for row in tabs]).astype(bool)
    store["s0"] = np.asarray(s0, dtype=np.int64)
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
