#!/usr/bin/env python3
"""Golden vectors for Sparse Sampling: the UNMODIFIED reference
``rl_agents.agents.tree_search.sparse_sampling.SparseSamplingAgent`` on deterministic, dense stochastic and sparse
finite-MDP tables.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_sparse_sampling.py      (build container only)

-> tests/golden/sparse_sampling.npz: per case the MDP, the planner's config, the generator record before and after
``plan()``, the plan, the root's chance values with their actions in listing order, the full tree (BFS listing, children in
creation order: parent, key, is_chance, depth, count, value) and ``len(planner.observations)``; or the exception the
reference raised.  Nothing of the reference is copied: inputs and its outputs only.

The reference's sparse_sampling.py predates numpy 2 and gymnasium; the adapters are make_golden_brue.py's, none of which
changes what it computes: ``np.infty`` (olop.py, which it imports), ``StaleGenerator.randint`` (:79), ``StaleApiEnv`` with
the 4-tuple ``step`` (:81) and ``seed(x)`` (:79) -> ``FiniteMDPEnv.seed(int(x))``, i.e. the clone's generator for a sample
is ``Generator(PCG64(SeedSequence(x)))``.  The env's tables are handed over as arrays, so that the reference's deep copy per
sample stays a memory copy.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401
from make_golden import agent_factory, bfs_tree, generators, np, put, put_mdp, rng_state  # noqa: E402
from make_golden_brue import StaleApiEnv, StaleGenerator  # noqa: E402  (also sets np.infty)

from rl_agents.agents.tree_search import sparse_sampling as ref_ss  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv  # noqa: E402
from rl_agents_amd.envs.finite_mdp import OrderedMaskedFiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "sparse_sampling.npz"))
SS = "<class 'rl_agents.agents.tree_search.sparse_sampling.SparseSamplingAgent'>"
SHIPPED = dict(gamma=0.7, horizon=3, C=3)       # scripts/configs/FiniteMDPEnv/agents/sparse_sampling.json
WIDE_FROM = 150                                 # the list-over-64 case: C is raised from here


def make_env(cfg, s0, available=None, order=None, max_steps=0):
    c = {k: (v if isinstance(v, str) else np.asarray(v)) for k, v in cfg.items()
         if k in ("mode", "transition", "reward", "terminal", "next")}
    c["state"], c["max_steps"] = int(s0), int(max_steps)
    if cfg.get("done_rule"):
        c["done_rule"] = cfg["done_rule"]
    if order is not None:
        env = OrderedMaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int), listing_order=list(order)))
    elif available is not None:
        env = MaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int)))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def tree_listing(root):
    chance = ref_ss.ChanceNode
    out = bfs_tree(root, [("is_chance", lambda n: isinstance(n, chance), np.uint8), ("depth", lambda n: n.depth, np.int32),
                          ("count", lambda n: 0 if isinstance(n, chance) else n.count, np.int64),
                          ("value", lambda n: float(n.value), np.float64)])
    out["key"] = out.pop("action")          # an action id under a decision node, the observed state under a chance node
    return out


def widest(root):
    todo, w = [root], 0
    while todo:
        n = todo.pop()
        if isinstance(n, ref_ss.ChanceNode):
            w = max(w, len(n.children))
        todo.extend(n.children.values())
    return w


def make_agent(cfg, s0, agent_cfg, seed, available=None, order=None, max_steps=0):
    env = make_env(cfg, s0, available, order, max_steps)
    agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=SS))
    agent.seed(seed)
    agent.planner.np_random = StaleGenerator(agent.planner.np_random.bit_generator)
    return agent


def one_plan(store, p, cfg, s0, agent_cfg, seed, available=None, order=None, max_steps=0, plans_before=0):
    agent = make_agent(cfg, s0, agent_cfg, seed, available, order, max_steps)
    planner = agent.planner
    for _ in range(plans_before):           # (step_strategy "reset": every plan starts on a new root)
        agent.plan(s0)
    n_actions = np.asarray(cfg["reward"]).shape[1]
    put_mdp(store, p + "/mdp", cfg)
    pc = planner.config
    put(store, p, dict(s0=s0, seed=seed, max_steps=max_steps, done_on_next=cfg.get("done_rule") == "next",
                       available=np.ones(np.asarray(cfg["reward"]).shape, bool) if available is None else available,
                       masked=available is not None, order=np.arange(n_actions) if order is None else np.asarray(order),
                       gamma=pc["gamma"], horizon=pc.get("horizon", -1), C=pc.get("C", -1), budget=pc["budget"],
                       step_strategy=pc["step_strategy"], plans_before=plans_before,
                       rng_before=rng_state(planner.np_random)))
    try:
        plan = agent.plan(s0)
    except Exception as e:
        put(store, p, dict(error=type(e).__name__, rng_after=rng_state(planner.np_random),
                           env_steps=len(planner.observations)))
        return None
    root = planner.root
    put(store, p, dict(error="", plan=np.asarray(plan, np.int32), rng_after=rng_state(planner.np_random),
                       env_steps=len(planner.observations), n_visits=len(planner.get_visits()),
                       root_actions=np.asarray(list(root.children.keys()), np.int32),
                       root_values=np.asarray([float(c.value) for c in root.children.values()], np.float64)))
    tree = tree_listing(root)
    put(store, p + "/tree", tree)
    return widest(root), len(tree["parent"])


def main():
    store, names = {}, []
    det = generators.random_deterministic(30, 3, seed=81)
    det_term = generators.random_deterministic(40, 3, seed=82, terminal_rate=0.3)
    dense = generators.random_stochastic(20, 3, seed=83)
    dense_next = dict(generators.random_stochastic(25, 4, seed=84, terminal_rate=0.2), done_rule="next")
    sparse = generators.random_sparse(60, 3, 2, seed=85)
    sparse_term = generators.random_sparse(50, 5, 3, seed=86, terminal_rate=0.15)
    sparse_next = dict(generators.random_sparse(50, 5, 3, seed=87, terminal_rate=0.15), done_rule="next")
    grid = generators.gridworld()
    grid01 = dict(grid, reward=(grid["reward"] > 0.5).astype(np.float64))          # 0/1 rewards: exact ties at the root
    one_sparse = generators.random_sparse(12, 1, 3, seed=88, terminal_rate=0.1)
    det5 = generators.random_deterministic(50, 5, seed=89, terminal_rate=0.1)
    avail5 = generators.random_available(50, 5, seed=90, rate=0.4)
    neg = generators.random_sparse(20, 3, 2, seed=91)
    neg["reward"] = np.asarray(neg["reward"]) * 5.0 - 2.0                          # no reward-range check
    negzero = generators.random_deterministic(12, 3, seed=92)
    nz = np.asarray(negzero["reward"], np.float64).copy()
    nz[np.random.default_rng(93).random(nz.shape) < 0.5] = -0.0
    negzero["reward"] = nz
    wide = generators.random_stochastic(100, 2, seed=94, concentration=1.0)
    root_term = int(np.flatnonzero(det_term["terminal"])[0])
    root_term_next = int(np.flatnonzero(sparse_next["terminal"])[0])
    cases = [
        # name, cfg, s0, agent config, seed, available, listing order, max_steps, plans before
        ("shipped_det", det, 0, SHIPPED, 0, None, None, 0, 0),
        ("shipped_sparse", sparse, 2, SHIPPED, 1, None, None, 0, 0),
        ("shipped_dense", dense, 1, SHIPPED, 2, None, None, 0, 0),
        ("horizon_1", sparse_term, 5, dict(gamma=0.9, horizon=1, C=4), 3, None, None, 0, 0),
        ("c1_h6_det", det, 4, dict(gamma=0.8, horizon=6, C=1), 4, None, None, 0, 0),
        ("grid01_ties", grid01, 0, dict(gamma=0.8, horizon=2, C=2), 5, None, None, 0, 0),
        ("grid01_near_goal", grid01, 66, dict(gamma=0.8, horizon=2, C=2), 6, None, None, 0, 0),
        ("one_action", one_sparse, 0, dict(gamma=0.9, horizon=3, C=3), 7, None, None, 0, 0),
        ("masked_ordered_det", det5, 3, dict(gamma=0.8, horizon=2, C=2), 8, avail5, [3, 0, 4, 1, 2], 0, 0),
        ("masked_ordered_sparse", sparse_term, 6, dict(gamma=0.8, horizon=2, C=3), 9, avail5, [2, 4, 0, 3, 1], 0, 0),
        ("masked_sorted_dense", dense_next, 3, dict(gamma=0.7, horizon=2, C=3), 10,
         generators.random_available(25, 4, seed=95, rate=0.4), None, 0, 0),
        ("negative_rewards", neg, 0, dict(gamma=0.8, horizon=2, C=3), 11, None, None, 0, 0),
        ("negative_zero_reward", negzero, 0, dict(gamma=0.9, horizon=2, C=2), 12, None, None, 0, 0),
        ("root_terminal_source", det_term, root_term, dict(gamma=0.8, horizon=3, C=2), 13, None, None, 2, 0),
        ("root_terminal_next_steplimit", sparse_next, root_term_next, dict(gamma=0.8, horizon=2, C=3), 14, None, None, 1, 0),
        ("terminals_inside_dense_next", dense_next, 0, dict(gamma=0.9, horizon=2, C=4), 15, None, None, 0, 0),
        ("odd_c_first_plan", sparse, 7, dict(gamma=0.9, horizon=1, C=5), 16, None, None, 0, 0),
        ("odd_c_second_plan", sparse, 7, dict(gamma=0.9, horizon=1, C=5), 16, None, None, 0, 1),
        ("odd_c_second_plan_h2", sparse, 9, dict(gamma=0.9, horizon=2, C=3), 17, None, None, 0, 1),
        ("c70_dense", dense, 0, dict(gamma=0.7, horizon=2, C=70), 18, None, None, 0, 0),
        ("missing_horizon", det, 0, dict(gamma=0.7, C=3), 19, None, None, 0, 0),
        ("missing_c", det, 0, dict(gamma=0.7, horizon=3), 20, None, None, 0, 0),
        ("horizon_0", det, 0, dict(gamma=0.7, horizon=0, C=3), 21, None, None, 0, 0),
        ("c_0", det, 0, dict(gamma=0.7, horizon=2, C=0), 22, None, None, 0, 0),
    ]
    for name, cfg, s0, agent_cfg, seed, avail, order, max_steps, before in cases:
        got = one_plan(store, "ss/" + name, cfg, s0, agent_cfg, seed, avail, order, max_steps, before)
        print(name, "error" if got is None else "widest list %d, %d nodes" % got, flush=True)
        names.append(name)

    # one case whose outcome list exceeds 64 at a level that is recursed into (the root's chance nodes at horizon 2): C is
    # raised until one of them lists more than 64 outcomes
    C = WIDE_FROM
    while True:
        agent = make_agent(wide, 0, dict(gamma=0.7, horizon=2, C=C), 23)
        agent.plan(0)
        w = max(len(c.children) for c in agent.planner.root.children.values())
        print("list_over_64: C", C, "width", w, flush=True)
        if w > 64:
            break
        C += 1
    got = one_plan(store, "ss/list_over_64", wide, 0, dict(gamma=0.7, horizon=2, C=C), 23)
    print("list_over_64", "widest list %d, %d nodes" % got, flush=True)
    names.append("list_over_64")
    store["ss/names"] = np.asarray(names)

    # one whole act() episode on a sparse model: a new plan per step (receding_horizon 1, step_strategy reset); the real
    # environment steps with its own seeded generator
    env = make_env(sparse_term, 5)
    env.seed(41)
    agent = agent_factory(StaleApiEnv(env), dict(SHIPPED, __class__=SS))
    agent.seed(40)
    agent.planner.np_random = StaleGenerator(agent.planner.np_random.bit_generator)
    st0 = rng_state(agent.planner.np_random)
    states, actions, rngs = [], [], []
    for _ in range(6):
        states.append(env.mdp.state)
        a = agent.act(env.mdp.state)
        agent.planner.np_random = StaleGenerator(agent.planner.np_random.bit_generator)
        actions.append(a)
        rngs.append(rng_state(agent.planner.np_random))
        env.step(a)
    put_mdp(store, "ss_episode/mdp", sparse_term)
    put(store, "ss_episode", dict(seed=40, env_seed=41, s0=5, rng_before=st0, states=np.asarray(states, np.int32),
                                  actions=np.asarray(actions, np.int32), rng_after=np.stack(rngs), **SHIPPED))
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
