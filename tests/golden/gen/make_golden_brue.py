#!/usr/bin/env python3
"""Golden vectors for BRUE: the UNMODIFIED reference ``rl_agents.agents.tree_search.brue.BRUEAgent`` on deterministic,
dense stochastic and sparse finite-MDP tables.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_brue.py      (build container only)

-> tests/golden/brue.npz: per case the MDP, the planner's config, the generator record before and after ``plan()``, the
plan, the full tree (BFS listing, children in creation order: parent, key, is_chance, depth, count and the running mean
-- ``reward`` of a decision node, ``value`` of a chance node), ``env_steps`` and ``get_visits()``; or the exception the
reference raised.  Nothing of the reference is copied: inputs and its outputs only.

The reference's brue.py predates numpy 2 and gymnasium.  Four adapters, none of which changes what it computes:

* ``np.infty`` (removed in numpy 2; olop.py, which brue.py imports, reads it) is aliased to ``np.inf`` before the
  reference is imported.
* ``self.np_random.randint(...)`` (brue.py:25,27): the planner's generator is a numpy ``Generator`` (gymnasium's
  ``seeding.np_random``), which has no ``randint``.  The generator is wrapped in a ``Generator`` subclass on the same
  bit generator whose ``randint`` is ``integers``: bounded draws that consume the stream like any other.
* ``next_observation, reward, done, _ = self.step(state, action)`` (brue.py:28): the 4-tuple of the old gym API.  The
  adapter folds the 5-tuple with ``done = terminated`` -- how the reference's current planners read it
  (deterministic.py:41) -- so a step limit (``truncated``) does not end a rollout.
* ``state.seed(x)`` (brue.py:25): gymnasium environments have no ``seed()``; the finite-MDP environment has, and the
  adapter forwards to it as ``seed(int(x))``: the clone's generator for the rollout is
  ``Generator(PCG64(SeedSequence(x)))``.  (The OLOP generator's ``seed`` does nothing: its tables are deterministic.)
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401
from make_golden import agent_factory, bfs_tree, generators, np, put, put_mdp, rng_state  # noqa: E402

np.infty = np.inf
from rl_agents.agents.tree_search import brue as ref_brue  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "brue.npz"))
BRUE = "<class 'rl_agents.agents.tree_search.brue.BRUEAgent'>"


class StaleGenerator(np.random.Generator):
    """numpy Generator with the legacy ``randint`` name (brue.py:25,27)."""
    randint = np.random.Generator.integers


class StaleApiEnv(object):
    """4-tuple ``step`` (done = terminated) and ``seed(x)`` -> the env's own ``seed(int(x))`` around a gymnasium-style
    finite-MDP env; everything else -- ``action_space``, ``get_available_actions`` when the env has it -- is the env's."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        env = self.__dict__.get("env")
        if env is None or name.startswith("__"):
            raise AttributeError(name)
        return getattr(env, name)

    def seed(self, seed=None):
        return self.env.seed(int(seed))

    def step(self, action):
        obs, reward, terminated, truncated, info = self.env.step(action)
        return obs, reward, terminated, info


def make_env(cfg, s0, available=None, max_steps=0):
    c = {k: v for k, v in cfg.items() if k in ("mode", "transition", "reward", "terminal", "next")}
    c = {k: (np.asarray(v).tolist() if not isinstance(v, str) else v) for k, v in c.items()}
    c["state"], c["max_steps"] = int(s0), int(max_steps)
    if cfg.get("done_rule"):
        c["done_rule"] = cfg["done_rule"]
    if available is not None:
        env = MaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def tree_listing(root):
    chance = ref_brue.ChanceNode
    out = bfs_tree(root, [("is_chance", lambda n: isinstance(n, chance), np.uint8), ("depth", lambda n: n.depth, np.int32),
                          ("count", lambda n: n.count, np.int64),
                          ("stat", lambda n: float(n.value if isinstance(n, chance) else n.reward), np.float64)])
    out["key"] = out.pop("action")          # an action id under a decision node, the observed state under a chance node
    return out


def one_plan(store, p, cfg, s0, agent_cfg, seed, available=None, max_steps=0):
    env = make_env(cfg, s0, available, max_steps)
    put_mdp(store, p + "/mdp", cfg)
    put(store, p, dict(s0=s0, seed=seed, max_steps=max_steps, done_on_next=cfg.get("done_rule") == "next",
                       available=np.ones(np.asarray(cfg["reward"]).shape, bool) if available is None else available))
    agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=BRUE))
    agent.seed(seed)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    pc = planner.config
    put(store, p, dict(budget=pc["budget"], gamma=pc["gamma"], horizon=pc["horizon"], episodes=pc.get("episodes", -1),
                       horizon_given="horizon" in agent_cfg, step_strategy=pc["step_strategy"],
                       rng_before=rng_state(planner.np_random)))
    try:
        plan = agent.plan(s0)
    except Exception as e:
        put(store, p, dict(error=type(e).__name__, rng_after=rng_state(planner.np_random),
                           env_steps=len(planner.observations)))
        return
    visits = planner.get_visits()
    keys = sorted(visits)
    put(store, p, dict(error="", plan=np.asarray(plan, np.int32), rng_after=rng_state(planner.np_random),
                       env_steps=len(planner.observations), visit_keys=np.asarray(keys, dtype=str),
                       visit_counts=np.asarray([visits[k] for k in keys], np.int64)))
    put(store, p + "/tree", tree_listing(planner.root))


def main():
    store, names = {}, []
    det = generators.random_deterministic(30, 3, seed=61)
    det_term = generators.random_deterministic(40, 3, seed=62, terminal_rate=0.3)
    det_next = dict(generators.random_deterministic(30, 4, seed=63, terminal_rate=0.2), done_rule="next")
    dense = generators.random_stochastic(20, 3, seed=64)
    dense_term = generators.random_stochastic(25, 4, seed=65, terminal_rate=0.2)
    dense_next = dict(generators.random_stochastic(25, 4, seed=66, terminal_rate=0.2), done_rule="next")
    sparse = generators.random_sparse(60, 3, 2, seed=67)
    sparse_term = generators.random_sparse(50, 5, 3, seed=68, terminal_rate=0.15)
    sparse_next = dict(generators.random_sparse(50, 5, 3, seed=69, terminal_rate=0.15), done_rule="next")
    grid = generators.gridworld()
    grid01 = dict(grid, reward=(grid["reward"] > 0.5).astype(np.float64))          # 0/1 rewards: exact ties at the root
    sparse01 = generators.random_sparse(30, 4, 2, seed=70)
    sparse01["reward"] = (np.asarray(sparse01["reward"]) > 0.6).astype(np.float64)
    one_det = generators.random_deterministic(10, 1, seed=71)
    one_sparse = generators.random_sparse(12, 1, 3, seed=72, terminal_rate=0.1)
    det5 = generators.random_deterministic(50, 5, seed=73, terminal_rate=0.1)
    avail5 = generators.random_available(50, 5, seed=74, rate=0.4)
    neg = generators.random_sparse(20, 3, 2, seed=75)
    neg["reward"] = np.asarray(neg["reward"]) * 5.0 - 2.0                          # no reward-range check in BRUE
    root_term = int(np.flatnonzero(det_term["terminal"])[0])
    root_term_next = int(np.flatnonzero(sparse_next["terminal"])[0])
    live_det = int(np.flatnonzero(~np.asarray(det_term["terminal"], bool))[0])
    live_one = int(np.flatnonzero(~np.asarray(one_sparse["terminal"], bool))[0])
    cases = [
        # name, cfg, s0, agent config, seed, available, max_steps
        ("det_default", det, 0, dict(budget=300, gamma=0.8), 0, None, 0),
        ("dense_default", dense, 1, dict(budget=300, gamma=0.8), 1, None, 0),
        ("sparse_1000_g09", sparse, 2, dict(budget=1000, gamma=0.9), 2, None, 0),
        ("det_terminal_source", det_term, live_det, dict(budget=200, gamma=0.85), 3, None, 0),
        ("det_terminal_next_steplimit", det_next, 4, dict(budget=150, gamma=0.7), 4, None, 3),
        ("dense_terminal_source", dense_term, 0, dict(budget=250, gamma=0.8), 5, None, 0),
        ("dense_terminal_next", dense_next, 3, dict(budget=250, gamma=0.7), 6, None, 0),
        ("sparse_terminal_source", sparse_term, 5, dict(budget=400, gamma=0.95), 7, None, 0),
        ("sparse_terminal_next", sparse_next, 6, dict(budget=400, gamma=0.8), 8, None, 0),
        ("root_terminal_source", det_term, root_term, dict(budget=40, gamma=0.8), 9, None, 0),
        ("root_terminal_next", sparse_next, root_term_next, dict(budget=40, gamma=0.8), 10, None, 0),
        ("grid01_ties", grid01, 0, dict(budget=60, gamma=0.8), 11, None, 0),
        ("grid01_near_goal", grid01, 55, dict(budget=300, gamma=0.8), 12, None, 0),
        ("sparse01_ties", sparse01, 3, dict(budget=12, gamma=0.7), 13, None, 0),
        ("one_action_det", one_det, 0, dict(budget=50, gamma=0.8), 14, None, 0),
        ("one_action_sparse", one_sparse, live_one, dict(budget=80, gamma=0.9), 15, None, 0),
        ("budget_below_actions", det5, 0, dict(budget=2, gamma=0.8), 16, None, 0),
        ("budget_one_dense", dense, 0, dict(budget=1, gamma=0.8), 17, None, 0),
        ("budget_zero", det, 0, dict(budget=0, gamma=0.8), 18, None, 0),
        ("given_horizon", sparse, 7, dict(budget=100, gamma=0.9, horizon=4), 19, None, 0),
        ("given_horizon_long", dense, 2, dict(budget=90, gamma=0.95, horizon=12), 20, None, 0),
        ("masked_env", det5, 3, dict(budget=250, gamma=0.8), 21, avail5, 0),
        ("det_g095_1000", det, 5, dict(budget=1000, gamma=0.95), 22, None, 0),
        ("negative_rewards", neg, 0, dict(budget=200, gamma=0.8), 23, None, 0),
    ]
    for name, cfg, s0, agent_cfg, seed, avail, max_steps in cases:
        one_plan(store, "brue/" + name, cfg, s0, agent_cfg, seed, avail, max_steps)
        names.append(name)
    store["brue/names"] = np.asarray(names)

    # one whole act() episode on a sparse model: a new plan per step (receding_horizon 1, step_strategy reset); the real
    # environment steps with its own seeded generator
    env = make_env(sparse_term, 5)
    env.seed(31)
    agent = agent_factory(StaleApiEnv(env), {"__class__": BRUE, "budget": 200, "gamma": 0.8})
    agent.seed(30)
    agent.planner.np_random = StaleGenerator(agent.planner.np_random.bit_generator)
    st0 = rng_state(agent.planner.np_random)
    states, actions, rngs = [], [], []
    for _ in range(8):
        states.append(env.mdp.state)
        a = agent.act(env.mdp.state)
        agent.planner.np_random = StaleGenerator(agent.planner.np_random.bit_generator)
        actions.append(a)
        rngs.append(rng_state(agent.planner.np_random))
        env.step(a)
    put_mdp(store, "brue_episode/mdp", sparse_term)
    put(store, "brue_episode", dict(seed=30, env_seed=31, s0=5, budget=200, gamma=0.8, rng_before=st0,
                                    states=np.asarray(states, np.int32), actions=np.asarray(actions, np.int32),
                                    rng_after=np.stack(rngs)))
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases")


if __name__ == "__main__":
    main()
