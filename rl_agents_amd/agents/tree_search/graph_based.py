"""GBOP-D, graph-based optimistic planning for deterministic systems, on the MI355X planning core (reference
``rl_agents/agents/tree_search/graph_based.py``); the epochs run in ``mp_gbopd_plan`` (rl_agents_amd/csrc/gbopd.hip).

What the reference's planner OBJECT keeps between ``plan()`` calls -- ``planner.nodes`` (one node per observed state with its
lower and upper bound, children and parents), ``updates_count`` and ``observations``; ``reset()`` only replaces ``root``
(graph_based.py:93-94) -- lives on the device in a ``native.GraphBasedPlanners`` batch that this planner holds for as long as
the model and the number of roots stay the same.  Consecutive ``plan()`` calls therefore continue on the same graph, across
``agent.reset()`` too, as a reference agent's do (tests/test_gpu_gbopd.py); changing the model or the batch size starts new
planners.  The parents of a node are kept in insertion order (the reference iterates a set hashed by address).
"""
import logging
from collections import defaultdict

import numpy as np

from rl_agents_amd import device_model, native
from rl_agents_amd.agents.tree_search.abstract import AbstractPlanner, AbstractTreeSearchAgent, Node

logger = logging.getLogger(__name__)


class GraphNode(Node):
    """One node of an exported graph (graph_based.py:12-81): ``observation`` (the state), ``value_lower`` / ``value_upper``,
    ``rewards`` and ``children`` by action in key order, ``parents`` (a list, in insertion order).  Read-only: the graph
    lives on the device; this is its picture after a plan."""

    def __init__(self, planner, observation, value_lower, value_upper, gamma=None):
        super(GraphNode, self).__init__(None, None, 0, value_lower, 0, planner)
        self.observation = observation
        self.value_lower, self.value_upper = value_lower, value_upper
        self.rewards = {}
        self.parents = []
        self._gamma = gamma

    def backup(self, field):
        """graph_based.py:55-58."""
        gamma = self._gamma if self.planner is None else self.planner.config["gamma"]
        return {a: self.rewards[a] + gamma * getattr(self.children[a], field) for a in self.children}

    def get_value(self):
        return self.value_lower

    def selection_rule(self):
        """Conservative action selection (graph_based.py:32-37): the first maximum of the lower backups."""
        if not self.children:
            return None
        q = self.backup("value_lower")
        return max(q, key=q.get)

    def sampling_rule(self):
        """Optimistic action (graph_based.py:22-30) without the tie draw: the first maximum (a viewer must not consume
        the planner's stream)."""
        if not self.children:
            return None
        q = self.backup("value_upper")
        return max(q, key=q.get)

    def get_trajectories(self, full_trajectories=True, include_leaves=True):
        return []                                               # graph_based.py:63-64

    def __str__(self):
        return "{} (L:{:.2f}, U:{:.2f})".format(str(self.observation), self.value_lower, self.value_upper)


def build_graph(listing, planner=None, gamma=None, order=None):
    """Creation-order arrays (native.GraphBasedPlanners.export, or the test restatement's listing) -> the reference's
    ``planner.nodes``: a dict of :class:`GraphNode` keyed by ``str(observation)`` in creation order.  ``order``: the
    environment's listing order when the model was loaded in the permuted action space (slot -> action id)."""
    nodes = [GraphNode(planner, int(s), float(lo), float(up), gamma)
             for s, lo, up in zip(listing["state"], listing["lower"], listing["upper"])]
    ptr, idx = listing["parent_ptr"], listing["parent_idx"]
    for i, node in enumerate(nodes):
        for k in range(int(listing["n_children"][i])):
            a = int(listing["child_action"][i, k])
            a = a if order is None else int(order[a])
            node.rewards[a] = float(listing["child_reward"][i, k])
            node.children[a] = nodes[int(listing["child_node"][i, k])]
        node.parents = [nodes[int(j)] for j in idx[ptr[i]:ptr[i + 1]]]
    return {str(node.observation): node for node in nodes}


class GraphBasedPlanner(AbstractPlanner):
    """GBOP-D planner (graph_based.py:84-138) for one or many independent planners of one deterministic finite MDP."""
    NODE_TYPE = GraphNode
    carries_state = True        # per-slot graphs on the device: callers keep the batch composition fixed
    supports_per_episode_tables = False   # PerEpisodeEvaluation: a kept graph was built on the previous step's table
    queue_capacity = None       # entries of a planner's backup queue on the device (None: MP_GBOPD_QUEUE, else the default)

    def __init__(self, env, config=None):
        self.env = env
        self._device = None     # (model, n_planners, native.GraphBasedPlanners)
        self._nodes = self._listing = None
        super(GraphBasedPlanner, self).__init__(config)

    def reset(self):
        """graph_based.py:93-94: a node is made, so ``1 / (1 - gamma)`` is evaluated -- gamma == 1 raises here, at
        construction.  Only the root is replaced: the graph and the counters stay."""
        self.value_max = 1 / (1 - self.config["gamma"])
        super(GraphBasedPlanner, self).reset()

    def step_by_subtree(self, action):
        """abstract.py:195-206 moves ``root`` to a child; ``plan`` installs the root by observation (:119): as reset."""
        self.step_by_reset()

    def device_planners(self, model, n):
        held = self._device
        if held is None or held[0] is not model or held[1] != n:
            if held is not None:
                logger.warning("graph-based planner: model or batch size changed (%d -> %d planners); the graph, bounds and "
                               "counters kept from earlier plans are dropped", held[1], n)
                held[2].close()
            held = self._device = (model, n, native.GraphBasedPlanners(self.models.ctx, model, n, self.queue_capacity))
            self._nodes = self._listing = None
        return held[2]

    def forget(self):
        """Drop the planners' kept graphs (a new planner object in the reference's terms)."""
        if self._device is not None:
            self._device[2].close()
            self._device = None
        self._nodes = self._listing = None

    # what the stochastic planner (rl_agents_amd/gbop.py), which plans through the same plan_batch, says differently
    kept_with_graph = "bounds and counters"     # what of a kept graph was built on the previous tables
    queue_knob = "MP_GBOPD_QUEUE"               # the environment knob its mp_*_create reads
    steps_count_when_raising = False            # GBOP: the reference's steps up to a failing step are taken before it raises

    def on_kept_graph(self, plan):
        """``plan()``, the one call of the kept planners; the library's refusal of tables that changed under them as the
        planner's own."""
        try:
            return plan()
        except native.NativeError as e:
            if "kept graph" in str(e):
                raise NotImplementedError("graph-based planner: the environment's tables changed; the graph, {} kept from earlier "
                                          "plans were built on the previous tables (call planner.forget() to start a new planner "
                                          "on the new ones)".format(self.kept_with_graph)) from e
            raise

    def plan_on(self, model, root_states, root_steps, rng_states, model_index=None, max_plan_len=None):
        """The one ``mp_gbopd_plan`` call.  ``root_steps`` is accepted for the common interface (the ``done`` flag of a step is
        discarded, :47); a batch model of one MDP per root is refused."""
        if model_index is not None:
            raise NotImplementedError("GBOP-D keeps its graph from plan to plan: one MDP per root is not planned")
        cfg = self.config
        planners = self.device_planners(model, len(root_states))
        self._nodes = self._listing = None
        return self.on_kept_graph(lambda: planners.plan(root_states, int(cfg["budget"]), cfg["gamma"], 1 / (1 - cfg["gamma"]),
                                                        cfg["accuracy"], int(cfg["sampling_timeout"]), rng_states))

    def plan_batch(self, state, root_states, root_steps=None, rng_states=None, keep_actions=None, env_rng_states=None):
        """``root_steps`` and ``keep_actions`` are accepted for the common interface ("subtree" equals "reset"), and so is
        ``env_rng_states``: GBOP-D plans on a deterministic table, and GBOP re-seeds every episode's clone with a draw of the
        planner's generator (graph_based_stochastic.py:239), so the environment's own generator is never read."""
        model = self.model_for(state)
        n = len(root_states)
        if rng_states is None:
            rng_states = self.batch_rng_states(n)
        out = self.plan_on(model, root_states, root_steps, rng_states)
        steps = int(out["env_steps"].sum())
        if self.steps_count_when_raising:
            self.env_steps += steps
        if not getattr(self, "defer_errors", False):               # (a batched caller checks its live slots only)
            self.raise_for_result(out)
        out["rng_states"] = rng_states
        out["root_lower"], out["root_upper"] = out["value_lower"], out["value_upper"]
        if out["plans"].ndim == 1:                                 # (GBOP: one action a root is a plan of length one)
            out["plans"] = out["plans"].reshape(n, 1)
        self.relabel(out, model)
        self.last, self._root, self._last_model = out, None, model
        if not self.steps_count_when_raising:
            self.env_steps += steps
        return out

    def plan(self, state, observation):
        """GraphBasedPlanner.plan (:118-124), with the planner's generator written back also when the plan raises."""
        s0, steps0 = device_model.env_root_state(state)
        rng = native.rng_state_from_generator(self.np_random).reshape(1, 6)
        try:
            out = self.plan_batch(state, [s0], [steps0], rng_states=rng)
        finally:
            native.generator_set_state(self.np_random, rng[0])
        n = int(out["plan_len"][0])
        return [int(a) for a in out["plans"][0, :n]]

    @classmethod
    def raise_for_status(cls, status):
        status = np.asarray(status)
        if (status == native.MP_ERR_ALLOC).any():
            raise RuntimeError("graph-based planner: backup queue overflow on the device; raise the queue capacity "
                               "({}.queue_capacity, or {} in the environment) and start again: the planner's graph is half "
                               "updated and stays failed".format(cls.__name__, cls.queue_knob))
        if (status == native.MP_ERR_GBOPD_NO_ACTION).any():         # np.amax([]) in partial_value_iteration (:74)
            raise ValueError("zero-size array to reduction operation maximum which has no identity")
        if (status == native.MP_ERR_GBOPD_DIVERGED).any():
            raise RuntimeError("graph-based planner: a plan made more than 2**22 queue pops without converging (accuracy 0 "
                               "with rewards outside [0, 1] lets the bounds cycle for ever: the reference never returns); "
                               "the planner's graph is half updated and stays failed")
        if (status != 0).any():
            raise RuntimeError("graph-based planner: the device refused the plan (status {}): a root state is out of "
                               "range".format(int(status[status != 0][0])))

    # -- the planner object's picture of the device graph (planner 0 of the batch)
    def export_graph(self, planner=0):
        """One planner's listing (mp_gbopd_export); planner 0's is kept until the next plan."""
        if self._device is None:
            return None
        if planner != 0:
            return self._device[2].export(planner)
        if self._listing is None:
            self._listing = self._device[2].export(0)
        return self._listing

    @property
    def nodes(self):
        """``planner.nodes`` (graph_based.py:89): GraphNode objects by ``str(observation)`` in creation order."""
        if self._device is None:
            return {}
        if self._nodes is None:
            self._nodes = build_graph(self.export_graph(0), self, order=self.action_order(self._device[0]))
        return self._nodes

    @property
    def root(self):
        if self._device is None or self.last is None:
            return None
        listing = self.export_graph(0)
        r = int(listing["root"])
        return None if r < 0 else self.nodes[str(int(listing["state"][r]))]

    def _counter(self, key):
        out = defaultdict(int)
        if self._device is not None:
            counts = self.export_graph(0)[key]
            for s in np.flatnonzero(counts):
                out[str(int(s))] = int(counts[s])
        return out

    def get_updates(self):
        """graph_based.py:137-138: ``updates_count`` over the planner's lifetime."""
        return self._counter("updates")

    def get_visits(self):
        """abstract.py:163-167 over the planner's lifetime (``observations`` is never cleared)."""
        return self._counter("visits")


class GraphBasedPlannerAgent(AbstractTreeSearchAgent):
    """Drop-in for ``rl_agents.agents.tree_search.graph_based.GraphBasedPlannerAgent``."""
    PLANNER_TYPE = GraphBasedPlanner

    @classmethod
    def default_config(cls):
        cfg = super(GraphBasedPlannerAgent, cls).default_config()
        cfg.update({"sampling_timeout": 100, "accuracy": 1e-2})
        return cfg
