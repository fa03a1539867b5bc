#!/usr/bin/env python3
"""Golden vectors for OLOP / KL-OLOP: the UNMODIFIED reference ``rl_agents.agents.tree_search.olop.OLOPAgent`` on
deterministic finite-MDP tables.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_olop.py      (build container only)

-> tests/golden/olop.npz: per case the MDP, the planner's config, the generator record before and after ``plan()``, the
plan, the full tree (BFS listing, children in creation order), ``env_steps`` and ``get_visits()``; or the exception the
reference raised.  Nothing of the reference is copied: inputs and its outputs only.

The reference's olop.py predates numpy 2 and gymnasium.  Four adapters, none of which changes what it computes:

* ``np.infty`` (removed in numpy 2) is aliased to ``np.inf`` before the reference is imported.
* ``self.np_random.randint(2**30)`` (olop.py:73): the planner's generator is a numpy ``Generator`` (gymnasium's
  ``seeding.np_random``), which has no ``randint``.  The generator is wrapped in a ``Generator`` subclass on the same
  bit generator whose ``randint`` is ``integers``: one bounded draw that consumes the stream like any other.
* ``state.seed(...)`` (olop.py:73): gymnasium environments have no ``seed()``.  The tables here are deterministic, so the
  adapter's ``seed`` does nothing.
* ``observation, reward, done, _ = self.step(state, action)`` (olop.py:88): the 4-tuple of the old gym API.  The
  adapter folds the 5-tuple with ``done = terminated`` -- how the reference's current planners read it
  (deterministic.py:41) -- so a step limit (``truncated``) does not end a node.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import agent_factory, bfs_tree, generators, np, put, put_mdp, rng_state  # noqa: E402

np.infty = np.inf
from rl_agents.agents.tree_search import olop as ref_olop  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "olop.npz"))
OLOP = "<class 'rl_agents.agents.tree_search.olop.OLOPAgent'>"
REF_CFG = os.path.join(mg.REF, "scripts", "configs")


class StaleGenerator(np.random.Generator):
    """numpy Generator with the legacy ``randint`` name (olop.py:73)."""
    randint = np.random.Generator.integers


class StaleApiEnv(object):
    """4-tuple ``step`` (done = terminated) and a no-op ``seed`` around a gymnasium-style finite-MDP env; everything
    else -- ``action_space``, ``get_available_actions`` when the env has it -- is the env's."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        env = self.__dict__.get("env")
        if env is None or name.startswith("__"):
            raise AttributeError(name)
        return getattr(env, name)

    def seed(self, seed=None):
        return [seed]

    def step(self, action):
        obs, reward, terminated, truncated, info = self.env.step(action)
        return obs, reward, terminated, info


def make_env(cfg, s0, available=None, order=None, max_steps=0):
    c = {k: v for k, v in cfg.items() if k in ("mode", "transition", "reward", "terminal")}
    c = {k: (np.asarray(v).tolist() if not isinstance(v, str) else v) for k, v in c.items()}
    c["state"], c["max_steps"] = int(s0), int(max_steps)
    if cfg.get("done_rule"):
        c["done_rule"] = cfg["done_rule"]
    if order is not None:
        env = OrderedMaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist(), listing_order=list(order)))
    elif available is not None:
        env = MaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def load_agent_json(rel):
    import json
    with open(os.path.join(REF_CFG, rel)) as f:
        cfg = json.load(f)
    cfg["__class__"] = OLOP
    return cfg


def tree_listing(root):
    return bfs_tree(root, [("depth", lambda n: n.depth, np.int32), ("count", lambda n: n.count, np.int64),
                           ("cum", lambda n: float(n.cumulative_reward), np.float64),
                           ("mu", lambda n: float(n.mu_ucb), np.float64), ("vu", lambda n: float(n.value_upper), np.float64),
                           ("done", lambda n: n.done, np.uint8)])


def record_config(store, p, pc):
    ub = pc["upper_bound"]
    put(store, p, dict(budget=pc["budget"], gamma=pc["gamma"], episodes=pc["episodes"], horizon=pc["horizon"],
                       bound_type=ub["type"], bound_time=ub.get("time", ""), threshold=ub.get("threshold", ""),
                       continuation=pc["continuation_type"]))


def one_plan(store, p, cfg, s0, agent_cfg, seed, available=None, order=None, max_steps=0):
    env = make_env(cfg, s0, available, order, max_steps)
    put_mdp(store, p + "/mdp", cfg)
    put(store, p, dict(s0=s0, seed=seed, max_steps=max_steps, done_on_next=cfg.get("done_rule") == "next",
                       available=np.ones(np.asarray(cfg["reward"]).shape, bool) if available is None else available,
                       order=np.arange(np.asarray(cfg["reward"]).shape[1]) if order is None else np.asarray(order)))
    try:
        agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=OLOP))
    except Exception as e:      # the reference builds its tree in reset(): some configs fail at construction
        put(store, p, dict(error=type(e).__name__, at="construction"))
        return
    agent.seed(seed)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    record_config(store, p, planner.config)
    st0 = rng_state(planner.np_random)
    put(store, p, dict(rng_before=st0))
    try:
        plan = agent.plan(s0)
    except Exception as e:
        put(store, p, dict(error=type(e).__name__, at="plan", rng_after=rng_state(planner.np_random),
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
    rnd = generators.random_deterministic(30, 3, seed=41)
    rnd_term = generators.random_deterministic(40, 3, seed=42, terminal_rate=0.3)
    grid = generators.gridworld()
    grid01 = dict(grid, reward=(grid["reward"] > 0.5).astype(np.float64))          # 0/1 rewards: exact ties
    rnd5 = generators.random_deterministic(50, 5, seed=43, terminal_rate=0.1)
    avail5 = generators.random_available(50, 5, seed=44, rate=0.4)
    bad = generators.random_deterministic(20, 3, seed=45)
    bad["reward"] = bad["reward"].copy()
    bad["reward"][:, 2] = 1.5
    nxt = dict(generators.random_deterministic(30, 4, seed=46, terminal_rate=0.2), done_rule="next")
    kl = {"type": "kullback-leibler"}
    fmdp_kl = load_agent_json("FiniteMDPEnv/agents/kl-olop.json")
    fmdp_olop = load_agent_json("FiniteMDPEnv/agents/olop.json")
    grid_kl = load_agent_json("GridWorld/agents/kl-olop.json")
    grid_kl1 = load_agent_json("GridWorld/agents/kl-olop-1.json")
    grid_olop = load_agent_json("GridWorld/agents/olop.json")
    grid_laplace = load_agent_json("GridWorld/agents/laplace.json")
    no0 = avail5.copy()
    no0[7, 0] = False
    no0[7, 1] = True
    cases = [
        # name, cfg, s0, agent config, seed, available, order, max_steps
        ("fmdp_kl_global", rnd, 0, fmdp_kl, 0, None, None, 0),
        ("fmdp_kl_local", rnd, 3, dict(fmdp_kl, upper_bound=dict(kl, time="local")), 1, None, None, 0),
        ("fmdp_olop_cfg", rnd, 0, fmdp_olop, 0, None, None, 0),        # "upper_bound": "hoeffding" (a string)
        ("fmdp_default_hoeffding", rnd, 5, dict(budget=100, gamma=0.9), 2, None, None, 0),
        ("grid_kl", grid, 0, grid_kl, 0, None, None, 0),
        ("grid_kl1", grid, 12, grid_kl1, 3, None, None, 0),
        ("grid_olop", grid, 44, grid_olop, 4, None, None, 0),
        ("grid_laplace", grid, 0, grid_laplace, 5, None, None, 0),
        ("grid01_kl_zeros", grid01, 55, dict(budget=300, gamma=0.8, upper_bound=kl), 6, None, None, 0),
        ("grid01_kl_uniform_local", grid01, 66, dict(budget=300, gamma=0.8, continuation_type="uniform",
                                                     upper_bound=dict(kl, time="local", threshold="2*np.log(time)")), 7, None, None, 0),
        ("terminal_kl_uniform", rnd_term, 1, dict(budget=200, gamma=0.85, continuation_type="uniform", upper_bound=kl), 8, None, None, 0),
        ("terminal_kl_zeros_steplimit", rnd_term, 2, dict(budget=200, gamma=0.85, upper_bound=kl), 9, None, None, 3),
        ("done_next_kl", nxt, 4, dict(budget=150, gamma=0.75, continuation_type="uniform", upper_bound=kl), 10, None, None, 0),
        ("masked_kl_uniform", rnd5, 3, dict(budget=250, gamma=0.8, continuation_type="uniform", upper_bound=kl), 11, avail5, None, 0),
        ("ordered_kl_uniform", rnd5, 3, dict(budget=250, gamma=0.8, continuation_type="uniform", upper_bound=kl), 12, avail5,
         [1, 0, 4, 2, 3], 0),
        ("ordered_hoeffding_uniform", rnd5, 9, dict(budget=120, gamma=0.9, continuation_type="uniform"), 13, avail5, [4, 3, 2, 1, 0], 0),
        ("masked_zeros_keyerror", rnd5, 7, dict(budget=100, gamma=0.8, upper_bound=kl), 14, no0, None, 0),
        ("reward_range", bad, 0, dict(budget=100, gamma=0.8, continuation_type="uniform", upper_bound=kl), 15, None, None, 0),
        ("given_horizon_kl", rnd, 6, dict(horizon=4, episodes=20, gamma=0.9, continuation_type="uniform", upper_bound=kl), 16,
         None, None, 0),
        ("small_budget", rnd5, 0, dict(budget=2, gamma=0.8, upper_bound=kl), 17, None, None, 0),   # max(A, budget)
    ]
    for name, cfg, s0, agent_cfg, seed, avail, order, max_steps in cases:
        one_plan(store, "olop/" + name, cfg, s0, {k: v for k, v in agent_cfg.items() if k != "__class__"}, seed, avail, order,
                 max_steps)
        names.append(name)
    store["olop/names"] = np.asarray(names)

    # one whole act() episode: KL-OLOP on the grid, a new plan per step (receding_horizon 1, step_strategy reset)
    env = make_env(grid, 0)
    agent = agent_factory(StaleApiEnv(env), dict(grid_kl))
    agent.seed(20)
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
    put_mdp(store, "olop_episode/mdp", grid)
    put(store, "olop_episode", dict(seed=20, rng_before=st0, states=np.asarray(states, np.int32),
                                    actions=np.asarray(actions, np.int32), rng_after=np.stack(rngs)))
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases")


if __name__ == "__main__":
    main()
