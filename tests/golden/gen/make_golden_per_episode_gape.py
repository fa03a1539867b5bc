#!/usr/bin/env python3
"""Golden vectors for MDP-GapE on a BATCH OF EPISODES WITH THEIR OWN, PER-STEP-CHANGING TABLES
(tests/golden/per_episode_gape.npz).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_per_episode_gape.py      (build container only)

As make_golden_per_episode_sparse_sampling.py: E + 1 episodes each own a highway-shaped (3, 4, 10) table that is REPLACED before
every step (as a re-extraction with to_finite_mdp() would), and the UNMODIFIED reference ``MDPGapEAgent`` -- one object per
episode, seeded 100 + e -- is driven step by step through the stale-API adapters of make_golden_olop.py, none of which changes
what it computes, with the ``Observers`` of make_golden_gape.py installed around every plan.  Tables, start states and seeds by
the rule of make_golden_per_episode.py (``table(e, t)``, start ``((e % V) * L + (e % L)) * TT``, seed 100 + e), with the rewards
CLIPPED to [1e-3, 1 - 1e-3]: on exact 0 and 1 rewards some plans compare bounds a few 1e-16 apart, which no device with another
``log`` can be held to.  Two configs: the reference's HighwayEnv/agents/MDPGapEAgent/baseline.json ("baseline") and a full run
of 32 episodes that never stops early ("full").

The script REFUSES to write a file unless every plan's smallest margin exceeds MARGIN, an episode ends by its own actions before
the last step, and every plan made a tie draw.  Per step: the plan, the generator record before and after it, ``episodes_run``,
``env_steps`` of this plan, and the root's arms in creation order (action, count, lower, upper); for one plan of each config the
whole tree listing of make_golden_gape.py.  Data only: inputs and outputs.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_gape import GAPE, MARGIN, Observers, load_agent_json, tree_listing  # noqa: E402  (np.infty is aliased first)
from make_golden_olop import StaleApiEnv, StaleGenerator  # noqa: E402
from make_golden import agent_factory, np, rng_state  # noqa: E402
from make_golden_per_episode import E, L, T_STEPS, TT, V, install, table  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "per_episode_gape.npz"))
CLIP = 1e-3
TREE_AT = (1, 1)                    # (episode, step) of the plan whose whole tree is stored: a table that has been replaced
CONFIGS = {
    "baseline": None,               # the reference's own JSON, read in main()
    "full": dict(horizon=4, episodes=30, gamma=0.8, accuracy=0.0,
                 upper_bound={"type": "kullback-leibler", "threshold": "1*np.log(time)"}),
}


def clipped(cfg):
    return dict(cfg, reward=np.clip(cfg["reward"], CLIP, 1 - CLIP))


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
    for k in ("gamma", "horizon", "episodes", "accuracy", "confidence", "budget"):
        store["{}/{}".format(name, k)] = np.asarray(pc[k])
    store["{}/continuation".format(name)] = np.asarray(pc["continuation_type"])
    store["{}/threshold".format(name)] = np.asarray(ub["threshold"])
    states, n_steps = [], 0
    for t in range(T_STEPS):
        install(env, tabs[t])
        s = env.mdp.state
        states.append(s)
        p = "{}/e{}/t{}".format(name, e, t)
        planner.np_random = StaleGenerator(planner.np_random.bit_generator)
        store[p + "/rng_before"] = rng_state(planner.np_random)
        steps_before = len(planner.observations)
        obs = Observers()
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
    CONFIGS["baseline"] = load_agent_json("HighwayEnv/agents/MDPGapEAgent/baseline.json")
    store = {}
    tabs = [[clipped(table(e, t)) for t in range(T_STEPS)] for e in range(E + 1)]
    s0 = [((e % V) * L + (e % L)) * TT for e in range(E + 1)]          # time slice 0 of some (speed, lane)
    for name, agent_cfg in CONFIGS.items():
        lengths, margins, draws = [], [], []
        for e in range(E + 1):
            arrays, n_steps, m, d = run_episode(name, agent_cfg, e, s0[e], tabs[e])
            store.update(arrays)
            lengths.append(n_steps)
            margins += m
            draws += d
        print("{:9s} steps {} smallest margin {:.3g} tie draws {}..{}".format(name, lengths, min(margins), min(draws), max(draws)))
        assert min(margins) > MARGIN, "{}: two compared values are {} apart".format(name, min(margins))
        assert min(lengths) < T_STEPS, "{}: no episode ends by its own actions before the last step".format(name)
        assert min(draws) >= 1, "{}: a plan without a tie draw".format(name)
        store["{}/margin".format(name)] = np.asarray(min(margins))
    store["configs"] = np.asarray(list(CONFIGS))
    store["transition"] = np.stack([np.stack([c["transition"] for c in row]) for row in tabs]).astype(np.int64)   # [E + 1,T,S,A]
    store["reward"] = np.stack([np.stack([c["reward"] for c in row]) for row in tabs]).astype(np.float64)
    store["terminal"] = np.stack([np.stack([c["terminal"] for c in row]) for row in tabs]).astype(bool)
    store["s0"] = np.asarray(s0, dtype=np.int64)
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
