"""GBOP, the graph-based optimistic planner for stochastic MDPs, on the MI355X planning core (reference
``rl_agents/agents/tree_search/graph_based_stochastic.py``); the episodes run in ``mp_gbop_plan`` (rl_agents_amd/csrc/gbop.hip;
DESIGN.md 4.14).

The classes are served by name from ``rl_agents_amd.agents.tree_search.graph_based_stochastic``, which is where an agent config
names them -- the reference's ``"__class__"`` line with only the package prefix changed::

    "<class 'rl_agents_amd.agents.tree_search.graph_based_stochastic.StochasticGraphBasedPlannerAgent'>"

They are defined in this module because the planner classes that modules of ``rl_agents_amd/agents`` define form a closed
table with what ``PerEpisodeEvaluation`` does with each; this planner inherits GBOP-D's refusal there (a kept graph).

What runs: every config whose reward threshold evaluates to 0 (``"threshold": "0*np.log(time)"``: every config the reference
ships) -- known rewards, a KL confidence region over transitions.  Any other value reaches the reference's mis-called
``kl_upper_bound`` and raises its ``TypeError`` here too, after the same draws and the same step.
"""
import logging
from collections import OrderedDict, defaultdict

import numpy as np

from rl_agents_amd import device_model, native
from rl_agents_amd.agents.tree_search.abstract import AbstractTreeSearchAgent, Node
from rl_agents_amd.agents.tree_search.graph_based import GraphBasedPlanner

logger = logging.getLogger(__name__)

PLACEHOLDERS_MESSAGE = ("No more placeholder nodes available, we observed more next states than "
                        "the 'max_next_states_count' config")                       # graph_based_stochastic.py:217-218
REWARD_THRESHOLD_MESSAGE = "kl_upper_bound() got multiple values for argument 'threshold'"   # :79-82
MAX_NEXT_STATES = 32                                                                 # a chance node's children fill half a wavefront


class ThresholdTables(object):
    """The config's two threshold strings by LIFETIME count (graph_based_stochastic.py:69-75, :200-205), extended by the new
    counts only: a kept graph's counts grow from plan to plan and the strings are never evaluated twice for a count."""

    def __init__(self):
        self.key = None
        self.reward = np.zeros(0, np.float64)
        self.transition = np.zeros(0, np.float64)
        self.evaluations = 0                   # counts evaluated so far (tests)

    def upto(self, bound, horizon, actions, episodes, n_counts):
        """Both tables with at least ``n_counts`` entries, ``[count - 1]``.  What an ``eval`` raises is raised as it is."""
        key = (bound["threshold"], bound["transition_threshold"], horizon, actions, episodes)
        if key != self.key:
            self.key, self.reward, self.transition = key, np.zeros(0, np.float64), np.zeros(0, np.float64)
        have = self.reward.size
        if n_counts > have:
            names = dict(horizon=horizon, actions=actions, time=episodes)
            new_r, new_t = np.empty(n_counts - have, np.float64), np.empty(n_counts - have, np.float64)
            for i, count in enumerate(range(have + 1, n_counts + 1)):
                new_r[i] = float(eval(bound["threshold"], {"np": np}, dict(names, count=count)))
                new_t[i] = float(eval(bound["transition_threshold"], {"np": np}, dict(names, count=count)))
            self.reward, self.transition = np.concatenate([self.reward, new_r]), np.concatenate([self.transition, new_t])
            self.evaluations += n_counts - have
        return self.reward, self.transition


class GraphDecisionNode(Node):
    """A decision node of an exported graph (graph_based_stochastic.py:15-130).  In ``planner.nodes`` it holds a state's
    ``count``, ``value_lower`` / ``value_upper``, ``children`` (action -> :class:`GraphChanceNode`, listing order) and
    ``parents`` (a list, in insertion order); as a child of a chance node it holds a transition's ``count``,
    ``cumulative_reward``, ``mu_ucb`` and ``mu_lcb``.  Read-only: the graph lives on the device."""

    def __init__(self, planner, observation, count=0, value_lower=0.0, value_upper=0.0):
        super(GraphDecisionNode, self).__init__(None, None, count, value_lower, 0, planner)
        self.observation = observation
        self.value_lower, self.value_upper = value_lower, value_upper
        self.cumulative_reward, self.mu_ucb, self.mu_lcb = 0, 1, 0
        self.parents = []

    def get_value(self):
        return self.value_lower

    def backup(self, field):
        return {a: getattr(c, field) for a, c in self.children.items()}

    def selection_rule(self):
        """:53-60 without the tie draw (a viewer must not consume the planner's stream): the first maximum of the stored
        lower bounds."""
        if not self.children:
            return None
        q = self.backup("value_lower")
        return max(q, key=q.get)

    def sampling_rule(self):
        if not self.children:
            return None
        q = self.backup("value_upper")
        return max(q, key=q.get)

    def get_field(self, field):
        """:118-124: the estimate of the state's representative in ``planner.nodes``."""
        nodes = {} if self.planner is None else self.planner.nodes
        return getattr(nodes.get(str(self.observation), self), field)

    def get_trajectories(self, full_trajectories=True, include_leaves=True):
        return []

    def __str__(self):
        return "{} (L:{:.2f}, U:{:.2f})".format(str(self.observation), self.value_lower, self.value_upper)


class GraphChanceNode(Node):
    """A chance node of an exported graph (:133-225): ``count``, ``value_lower`` / ``value_upper`` (the stored bounds),
    ``children`` (key -> transition child, the reference's dict order: the placeholders left, then the observed states by first
    observation), ``p_hat``, and ``p_plus`` / ``p_minus`` / ``next_states`` as the last backup left them (None before one)."""

    def __init__(self, planner, parent, count, value_lower, value_upper):
        super(GraphChanceNode, self).__init__(None, None, count, value_upper, 0, planner)
        self.parent = parent
        self.value_lower, self.value_upper = value_lower, value_upper
        self.children = OrderedDict()
        self.p_hat = self.p_plus = self.p_minus = self.next_states = None

    def get_value(self):
        return self.value_upper

    def get_trajectories(self, full_trajectories=True, include_leaves=True):
        return []

    def __str__(self):
        return "{} (L:{:.2f}, U:{:.2f})".format(id(self), self.value_lower, self.value_upper)


def key_label(key):
    key = int(key)
    return "placeholder_{}".format(-1 - key) if key < 0 else str(key)


def build_graph(listing, planner=None, order=None):
    """Creation-order arrays (native.StochasticGraphBasedPlanners.export, or the test restatement's listing) -> the
    reference's ``planner.nodes``: :class:`GraphDecisionNode` objects keyed by ``str(observation)`` in creation order.
    ``order``: the environment's listing order when the model was loaded in the permuted action space (slot -> action id)."""
    nodes = [GraphDecisionNode(planner, int(s), int(c), float(lo), float(up))
             for s, c, lo, up in zip(listing["state"], listing["count"], listing["lower"], listing["upper"])]
    ptr, idx = listing["parent_ptr"], listing["parent_idx"]
    K = listing["k_state"].shape[2] if len(nodes) else 0
    for i, node in enumerate(nodes):
        for k in range(int(listing["n_children"][i])):
            a = int(listing["action"][i, k])
            a = a if order is None else int(order[a])
            ch = GraphChanceNode(planner, node, int(listing["c_count"][i, k]), float(listing["c_lower"][i, k]),
                                 float(listing["c_upper"][i, k]))
            for j in range(K):
                key = int(listing["k_state"][i, k, j])
                d = GraphDecisionNode(planner, "placeholder" if key < 0 else key, int(listing["k_count"][i, k, j]))
                d.cumulative_reward = float(listing["k_cum"][i, k, j])
                d.mu_ucb, d.mu_lcb = float(listing["k_mu_ucb"][i, k, j]), float(listing["k_mu_lcb"][i, k, j])
                ch.children[key_label(key)] = d
            if ch.count:
                ch.p_hat = listing["k_count"][i, k] / ch.count
            backed = int(listing["c_backed"][i, k])
            if backed >= 0:
                ch.p_plus, ch.p_minus = listing["p_plus"][i, k].copy(), listing["p_minus"][i, k].copy()
                # the dict order when the backup ran: the placeholders backed .. K - 1, then the first `backed` states
                assigned = [lbl for lbl in ch.children if not lbl.startswith("placeholder_")]
                ch.next_states = ["placeholder_{}".format(j) for j in range(backed, K)] + assigned[:backed]
            node.children[a] = ch
        node.parents = [nodes[int(j)] for j in idx[ptr[i]:ptr[i + 1]]]
    return {str(node.observation): node for node in nodes}


class StochasticGraphBasedPlanner(GraphBasedPlanner):
    """GBOP planner (graph_based_stochastic.py:228-343) for one or many independent planners of one finite MDP: a
    deterministic table, a ``stochastic`` [S, A, S] or a ``sparse`` [S, A, B] model, with or without an availability table and
    listing order.  The graph, every count and every chance record live on the device in a
    ``native.StochasticGraphBasedPlanners`` batch from plan to plan, across ``agent.reset()`` too; :meth:`forget` starts over.

    Refused: ``max_next_states_count`` above 32 (NotImplementedError) or below 1 (ValueError), a bound type other than
    ``"kullback-leibler"`` (the reference only logs an error and plans on the initial reward bounds), one model per episode
    (``supports_per_episode_tables`` False), CartPole models."""
    NODE_TYPE = GraphDecisionNode
    carries_state = True
    supports_per_episode_tables = False
    per_episode_kind = None
    kept_with_graph = "counts and chance records"
    queue_knob = "MP_GBOP_QUEUE"                # (mp_gbop_create reads its own knob)
    steps_count_when_raising = True             # the reference's steps and draws up to a failing step are taken before it raises

    def __init__(self, env, config=None):
        self.tables = ThresholdTables()
        super(StochasticGraphBasedPlanner, self).__init__(env, config)

    def reset(self):
        """:339-343: a node is made (``1 / (1 - gamma)``: ZeroDivisionError for gamma == 1), only the root is replaced, and
        without ``"horizon"`` in the config the budget is split as OLOP splits it."""
        super(StochasticGraphBasedPlanner, self).reset()
        if "horizon" not in self.config:
            budget = max(self.env.action_space.n, self.config["budget"])
            self.config["episodes"], self.config["horizon"] = native.olop_allocation(budget, self.config["gamma"])

    def supports_device_loop(self):
        return False

    def model_for(self, state):
        """Deterministic, ``stochastic`` and ``sparse`` finite MDPs with the env's availability table, the columns in the
        env's listing order (expand asks the state which actions it lists, :107-113)."""
        if device_model.is_cartpole(state):
            raise TypeError("this planner needs a finite-MDP environment")
        mdp = device_model.finite_mdp_of(state)
        if mdp.mode == "deterministic":
            return super(StochasticGraphBasedPlanner, self).model_for(state)
        available, order = device_model.availability_of(state, mdp)
        spec = device_model.spec_from_mdp(mdp, available=available, action_order=order)
        model = self.models.get(spec)
        if spec.available is not None and getattr(model, "available", None) is None:
            model.set_available(spec.available)
        return model

    def next_states_count(self):
        count = self.config["max_next_states_count"]
        if count != int(count) or int(count) < 1:
            raise ValueError("max_next_states_count {}: a chance node needs a placeholder for its first next state".format(count))
        if count > MAX_NEXT_STATES:
            raise NotImplementedError("max_next_states_count {} > {}: a chance node's children fill half a wavefront on the "
                                      "device".format(count, MAX_NEXT_STATES))
        return int(count)

    def device_planners(self, model, n):
        held, K = self._device, self.next_states_count()
        if held is None or held[0] is not model or held[1] != n or held[2].K != K:
            if held is not None:
                logger.warning("graph-based planner: model, batch size or max_next_states_count changed (%d -> %d planners); the "
                               "graph, counts and chance records kept from earlier plans are dropped", held[1], n)
                held[2].close()
            held = self._device = (model, n, native.StochasticGraphBasedPlanners(self.models.ctx, model, n, K,
                                                                                 self.queue_capacity))
            self._nodes = self._listing = None
        return held[2]

    def plan_on(self, model, root_states, root_steps, rng_states, model_index=None, max_plan_len=None):
        """The thresholds by lifetime count from the config and the one ``mp_gbop_plan`` call.  ``root_steps`` is accepted for
        the common interface (``done`` is discarded, :251); a batch model of one MDP per root is refused."""
        if model_index is not None:
            raise NotImplementedError("GBOP keeps its graph from plan to plan: one MDP per root is not planned")
        cfg = self.config
        bound = cfg["upper_bound"]
        if bound["type"] != "kullback-leibler":
            raise ValueError("GBOP needs the 'kullback-leibler' bound: with '{}' the reference only logs an error and plans on "
                             "the initial reward bounds".format(bound["type"]))
        episodes, horizon = int(cfg["episodes"]), int(cfg["horizon"])
        planners = self.device_planners(model, len(root_states))
        self._nodes = self._listing = None
        reach = planners.info()["max_count"] + episodes * horizon
        reward, transition = self.tables.upto(bound, cfg["horizon"], self.env.action_space.n, cfg["episodes"], reach)
        return self.on_kept_graph(lambda: planners.plan(
            root_states, episodes, horizon, cfg["gamma"], 1 / (1 - cfg["gamma"]), cfg["accuracy"], int(cfg["sampling_timeout"]),
            reward[:reach], transition[:reach], rng_states))

    @classmethod
    def raise_for_status(cls, status):
        status = np.asarray(status)
        if (status == native.ERR_GBOP_PLACEHOLDERS).any():
            raise ValueError(PLACEHOLDERS_MESSAGE)
        if (status == native.ERR_GBOP_REWARD_THRESHOLD).any():
            raise TypeError(REWARD_THRESHOLD_MESSAGE)
        if (status == native.ERR_GBOP_CHOICE_P).any():
            raise ValueError("probabilities do not sum to 1")                       # Generator.choice in get_plan (:156)
        super(StochasticGraphBasedPlanner, cls).raise_for_status(status)        # (a full queue first, under this class's names)

    def _plan_of(self, out, i=0):
        n = int(out["plan_len"][i])
        plan = [int(out["plans"][i, 0])] if n >= 1 else []
        if n >= 2:
            plan.append(key_label(out["key"][i]))
        return plan

    def plan(self, state, observation):
        """StochasticGraphBasedPlanner.plan (:332-337) -> the reference's list ``[action, key]``, the key a string; the
        planner's generator is written back also when the plan raises."""
        s0, steps0 = device_model.env_root_state(state)
        rng = native.rng_state_from_generator(self.np_random).reshape(1, 6)
        try:
            out = self.plan_batch(state, [s0], [steps0], rng_states=rng)
        finally:
            native.generator_set_state(self.np_random, rng[0])
        return self._plan_of(out)

    def get_plan(self):
        return [] if self.last is None else self._plan_of(self.last)

    @property
    def nodes(self):
        """``planner.nodes``: :class:`GraphDecisionNode` objects by ``str(observation)`` in creation order (planner 0)."""
        if self._device is None:
            return {}
        if self._nodes is None:
            self._nodes = build_graph(self.export_graph(0), self, order=self.action_order(self._device[0]))
        return self._nodes

    def get_updates(self):
        """``updates_count`` is never touched by this planner's partial value iteration (:89-101)."""
        return defaultdict(int)


class StochasticGraphBasedPlannerAgent(AbstractTreeSearchAgent):
    """Drop-in for ``rl_agents.agents.tree_search.graph_based_stochastic.StochasticGraphBasedPlannerAgent``."""
    PLANNER_TYPE = StochasticGraphBasedPlanner

    @classmethod
    def default_config(cls):
        cfg = super(StochasticGraphBasedPlannerAgent, cls).default_config()
        cfg.update({
            "sampling_timeout": 100,
            "accuracy": 1e-2,
            "max_next_states_count": 1,
            "upper_bound": {
                "type": "kullback-leibler",
                "time": "global",
                "threshold": "1*np.log(time)",
                "transition_threshold": "0.1*np.log(time)"
            },
        })
        return cfg
