#!/usr/bin/env python3
"""Golden vectors for GBOP-D: the UNMODIFIED reference ``rl_agents.agents.tree_search.graph_based.GraphBasedPlannerAgent``
on deterministic finite-MDP tables.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_gbopd.py      (build container only)

-> tests/golden/gbopd.npz.  Per case: the MDP, the availability table and listing order of the environment, the config, the
seed; per ``plan()`` of the case the root, the generator record before and after, the plan (or the exception type) and the
planner's whole graph afterwards -- the nodes in creation order (state, both bounds, expanded, children and rewards in key
order, parents in order), ``get_updates()``, ``get_visits()`` and ``len(observations)``.  Nothing of the reference is copied:
inputs and its outputs only.  The file is written with fixed zip timestamps: two runs give identical bytes.

Two adapters, neither of which changes what the reference computes:

* ``next_observation, reward, done, _ = self.planner.step(state, action)`` (graph_based.py:47): the 4-tuple of the old gym
  API.  ``StaleApiEnv`` (make_golden_brue.py) folds the 5-tuple with ``done = terminated``; the flag is discarded anyway.
* ``queue.extend(list(node.parents))`` (graph_based.py:78) iterates a ``set`` of nodes hashed by ADDRESS: the reference's own
  order is unspecified, and it changes bounds, update counts and plans.  This project defines it as INSERTION order (the
  order in which parents first expanded into the node).  ``OrderedParentsNode`` -- a ``GraphNode`` subclass installed as
  ``GraphBasedPlanner.NODE_TYPE`` -- replaces ``parents`` by a dict-backed set with ``add`` and insertion-order iteration;
  nothing else is overridden.
"""
import io
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401
from make_golden import agent_factory, generators, np, put, put_mdp, rng_state  # noqa: E402
from make_golden_brue import StaleApiEnv  # noqa: E402

from rl_agents.agents.tree_search import graph_based as ref_gb  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "gbopd.npz"))
GBOPD = "<class 'rl_agents.agents.tree_search.graph_based.GraphBasedPlannerAgent'>"


class InsertionOrderedSet(object):
    """``add`` + iteration in insertion order (a dict's keys)."""

    def __init__(self):
        self._items = {}

    def add(self, item):
        self._items.setdefault(item, None)

    def __iter__(self):
        return iter(self._items)

    def __len__(self):
        return len(self._items)


class OrderedParentsNode(ref_gb.GraphNode):
    def __init__(self, planner, state, observation):
        super().__init__(planner, state, observation)
        self.parents = InsertionOrderedSet()


def install_adapter():
    ref_gb.GraphBasedPlanner.NODE_TYPE = OrderedParentsNode


def make_env(cfg, s0, available=None, order=None):
    c = {k: v for k, v in cfg.items() if k in ("mode", "transition", "reward", "terminal")}
    c = {k: (np.asarray(v).tolist() if not isinstance(v, str) else v) for k, v in c.items()}
    c["state"], c["max_steps"] = int(s0), 0
    if order is not None:
        env = OrderedMaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist(), listing_order=list(order)))
    elif available is not None:
        env = MaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def graph_listing(planner, n_states, n_actions):
    nodes = list(planner.nodes.values())                 # creation order
    index = {id(n): i for i, n in enumerate(nodes)}
    n = len(nodes)
    child_action = np.full((n, n_actions), -1, np.int32)
    child_node = np.full((n, n_actions), -1, np.int32)
    child_reward = np.zeros((n, n_actions), np.float64)
    n_children = np.zeros(n, np.int32)
    parent_ptr, parent_idx = [0], []
    for i, node in enumerate(nodes):
        for k, (a, child) in enumerate(node.children.items()):       # key order
            child_action[i, k], child_node[i, k], child_reward[i, k] = int(a), index[id(child)], float(node.rewards[a])
        n_children[i] = len(node.children)
        parent_idx.extend(index[id(p)] for p in node.parents)
        parent_ptr.append(len(parent_idx))
    updates, visits = np.zeros(n_states, np.int64), np.zeros(n_states, np.int64)
    for k, v in planner.get_updates().items():
        updates[int(k)] = v
    for k, v in planner.get_visits().items():
        visits[int(k)] = v
    return dict(state=np.asarray([int(x.observation) for x in nodes], np.int32),
                lower=np.asarray([float(x.value_lower) for x in nodes], np.float64),
                upper=np.asarray([float(x.value_upper) for x in nodes], np.float64),
                expanded=np.asarray([bool(x.children) for x in nodes], np.uint8),
                n_children=n_children, child_action=child_action, child_node=child_node, child_reward=child_reward,
                parent_ptr=np.asarray(parent_ptr, np.int32), parent_idx=np.asarray(parent_idx, np.int32),
                updates=updates, visits=visits, n_observations=len(planner.observations),
                root=index[id(planner.root)] if id(planner.root) in index else -1)


def run_case(store, name, cfg, agent_cfg, seed, script, available=None, order=None):
    """``script``: a list of ("plan", s) -- put the environment in state s and call agent.plan(s) --, ("act", s) -- the same
    through agent.act --, ("act",) -- agent.act in the environment's current state, then env.step(action) -- and
    ("reset", s): agent.reset() and the environment put in state s."""
    p = "gbopd/" + name
    reward = np.asarray(cfg["reward"], np.float64)
    S, A = reward.shape
    put_mdp(store, p + "/mdp", cfg)
    put(store, p, dict(seed=seed, available=np.ones((S, A), bool) if available is None else np.asarray(available, bool),
                       order=np.arange(A) if order is None else np.asarray(order), masked=available is not None,
                       ordered=order is not None))
    env = make_env(cfg, 0, available, order)
    try:
        agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=GBOPD))
    except Exception as e:
        put(store, p, dict(construct_error=type(e).__name__, n_plans=0, gamma=agent_cfg.get("gamma", 0.8)))
        return
    agent.seed(seed)
    planner = agent.planner
    pc = planner.config
    put(store, p, dict(construct_error="", budget=pc["budget"], gamma=pc["gamma"], accuracy=pc["accuracy"],
                       sampling_timeout=pc["sampling_timeout"], step_strategy=pc["step_strategy"]))
    roots, via_act, reset_before = [], [], []
    pending_reset = False
    i = 0
    for op in script:
        if op[0] == "reset":
            agent.reset()
            env.mdp.state = int(op[1])
            pending_reset = True
            continue
        if len(op) > 1:
            env.mdp.state = int(op[1])
        s = int(env.mdp.state)
        q = "{}/plan{}".format(p, i)
        store[q + "/rng_before"] = rng_state(planner.np_random)
        error, plan = "", []
        try:
            if op[0] == "act":
                plan = [agent.act(s)]
                plan = list(agent.previous_actions)
            else:
                plan = agent.plan(s)
        except Exception as e:
            error = type(e).__name__
        put(store, q, dict(error=error, plan=np.asarray(plan, np.int32), rng_after=rng_state(planner.np_random)))
        put(store, q + "/graph", graph_listing(planner, S, A))
        roots.append(s); via_act.append(op[0] == "act"); reset_before.append(pending_reset)
        pending_reset = False
        i += 1
        if op[0] == "act" and not error:
            env.step(plan[0])
    put(store, p, dict(n_plans=i, roots=np.asarray(roots, np.int32), via_act=np.asarray(via_act, bool),
                       reset_before=np.asarray(reset_before, bool)))


def save_npz(path, store):
    """np.savez_compressed with fixed member timestamps (identical bytes on every run)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(store[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def cases():
    grid = generators.gridworld()
    det = generators.random_deterministic(50, 4, seed=81)
    det_term = generators.random_deterministic(60, 3, seed=82, terminal_rate=0.2)
    hw = generators.highway_shaped(3, 4, 10, seed=3)
    many = generators.random_deterministic(40, 70, seed=83)
    many_ties = dict(many, reward=np.round(np.asarray(many["reward"]) * 2) / 2)     # rewards 0, 0.5, 1: ties over 70 actions
    det5 = generators.random_deterministic(50, 5, seed=84, terminal_rate=0.1)
    avail5 = generators.random_available(50, 5, seed=85, rate=0.4)
    small = generators.random_deterministic(20, 3, seed=1)
    det8 = generators.random_deterministic(50, 8, seed=86)
    equal = generators.random_deterministic(30, 4, seed=87)
    equal = dict(equal, reward=np.full_like(np.asarray(equal["reward"], np.float64), 0.5))
    neg = generators.random_deterministic(40, 4, seed=88)
    neg = dict(neg, reward=np.asarray(neg["reward"]) * 5.0 - 2.0)                    # no reward-range check in GBOP-D
    idle_first = [1, 0, 4, 2, 3]
    episode = [("act", 0)] + [("act",)] * 8 + [("reset", 93)] + [("act",)] * 9
    return [
        # name, mdp, agent config, seed, script, available, listing order
        ("grid_default", grid, dict(budget=400), 0, [("plan", 0)], None, None),
        ("grid_g09_acc1e3", grid, dict(budget=400, gamma=0.9, accuracy=1e-3), 1, [("plan", 55), ("plan", 55)], None, None),
        ("grid_timeout10", grid, dict(budget=400, gamma=0.95, sampling_timeout=10), 2, [("plan", 12), ("plan", 13)], None, None),
        ("det_g095", det, dict(budget=300, gamma=0.95), 3, [("plan", 0), ("plan", 7)], None, None),
        ("det_terminal", det_term, dict(budget=300, gamma=0.8), 4, [("plan", 1), ("plan", 2)], None, None),
        ("highway", hw, dict(budget=300, gamma=0.8), 5, [("plan", 0), ("plan", 41)], None, None),
        ("many_actions", many, dict(budget=700, gamma=0.8), 6, [("plan", 0), ("plan", 3)], None, None),
        ("many_actions_ties", many_ties, dict(budget=1400, gamma=0.9, accuracy=1e-3), 7, [("plan", 2), ("plan", 2)], None, None),
        ("masked", det5, dict(budget=250, gamma=0.8), 8, [("plan", 3), ("plan", 9)], avail5, None),
        ("ordered_masked", det5, dict(budget=250, gamma=0.9), 9, [("plan", 3), ("plan", 4)], avail5, idle_first),
        ("full_expansion", small, dict(budget=400, gamma=0.8), 10, [("plan", 0), ("plan", 5)], None, None),
        ("full_expansion_timeout10", small, dict(budget=400, gamma=0.9, sampling_timeout=10), 11, [("plan", 0), ("plan", 0)], None, None),
        ("accuracy_zero", small, dict(budget=60, gamma=0.8, accuracy=0), 12, [("plan", 0)], None, None),
        ("accuracy_one", det, dict(budget=300, gamma=0.9, accuracy=1.0), 13, [("plan", 0), ("plan", 1)], None, None),
        ("gamma099_acc1e4", det8, dict(budget=240, gamma=0.99, accuracy=1e-4), 14, [("plan", 0)], None, None),
        ("gamma099", det8, dict(budget=400, gamma=0.99), 15, [("plan", 5), ("plan", 6)], None, None),
        ("equal_rewards", equal, dict(budget=200, gamma=0.8), 16, [("plan", 0), ("plan", 0), ("plan", 4)], None, None),
        ("budget_below_actions", det5, dict(budget=3, gamma=0.8), 17, [("plan", 0), ("act", 0)], None, None),
        ("rewards_outside_unit", neg, dict(budget=200, gamma=0.8), 18, [("plan", 0), ("plan", 3)], None, None),
        ("episodes_reset", grid, dict(budget=200, gamma=0.9), 19, episode, None, None),
        ("episodes_subtree", grid, dict(budget=200, gamma=0.9, step_strategy="subtree"), 19, episode, None, None),
        ("gamma_one", small, dict(budget=60, gamma=1), 20, [], None, None),
    ]


def main():
    install_adapter()
    store, names = {}, []
    for name, cfg, agent_cfg, seed, script, avail, order in cases():
        run_case(store, name, cfg, agent_cfg, seed, script, avail, order)
        names.append(name)
        print(name, flush=True)
    store["gbopd/names"] = np.asarray(names)
    save_npz(OUT, store)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
