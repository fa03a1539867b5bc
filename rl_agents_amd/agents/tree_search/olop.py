"""Open-Loop Optimistic Planning, OLOP / KL-OLOP, on the MI355X planning core (reference
``rl_agents/agents/tree_search/olop.py``); the episodes run in ``mp_olop_plan`` (rl_agents_amd/csrc/olop.hip).

Same class names, config keys and results as the reference on deterministic finite-MDP tables (``OLOPAgent``) and, through
``mp_olop_plan_stochastic``, on ``stochastic`` [S, A, S] and ``sparse`` [S, A, B] models too (``StochasticOLOPAgent``): the
clone re-seeded per episode, the state carried by the episode, a node's children fixed at its first expansion.  What the host
computes:
the budget split (``allocation``, also used by MCTS), the initial upper bounds by depth (Python ``**``) and the bound's
threshold per episode (``eval`` of the config string) -- every constant that is not a basic IEEE operation.  The
device computes the KL bound's Newton iteration with its own ``log``: bounds agree with the reference within 1e-12 and
every discrete output is identical.
"""
import logging

import numpy as np

from rl_agents_amd import device_model, native
from rl_agents_amd.agents.tree_search.abstract import AbstractPlanner, AbstractTreeSearchAgent, Node

logger = logging.getLogger(__name__)


class OLOP(AbstractPlanner):
    """OLOP planner (olop.py:11-100) for one or many roots of one finite MDP."""

    def __init__(self, env, config=None):
        self.env = env
        super(OLOP, self).__init__(config)

    @classmethod
    def default_config(cls):
        cfg = super(OLOP, cls).default_config()
        cfg["upper_bound"] = dict(type="hoeffding", time="global", threshold="4*np.log(time)")
        cfg["continuation_type"] = "zeros"
        return cfg

    def reset(self):
        """olop.py:36-40.  The reference builds its root here, so what that raises is raised here: a non-mapping
        ``upper_bound`` (TypeError), ``gamma == 1`` (ValueError from the allocation, ZeroDivisionError with a given horizon)."""
        super(OLOP, self).reset()
        if self.config["step_strategy"] == "subtree":
            # on a kept subtree the reference walks past the horizon and fails the assert of olop.py:190
            raise NotImplementedError("step_strategy 'subtree' is not available for OLOP")
        if "horizon" not in self.config:
            self.allocate_budget()
        bound = self.config["upper_bound"]
        bound["type"]                                   # olop.py:107 reads it: TypeError for "upper_bound": "hoeffding"
        self._value_upper_init = self.value_upper_init(self.config["gamma"], self.config["horizon"])

    @staticmethod
    def horizon(episodes, gamma):
        """L(M) = max(1, ceil(log M / (2 log(1 / gamma)))) in numpy arithmetic (olop.py:42-44): gamma == 1 gives int(nan)."""
        denominator = 2 * np.log(1 / gamma)
        length = np.ceil(np.log(episodes) / denominator)
        return max(int(length), 1)

    def allocate_budget(self):
        """olop.py:46-48: the budget is at least the number of actions."""
        n_actions = self.env.action_space.n
        budget = self.config["budget"] if self.config["budget"] > n_actions else n_actions
        # the reference's first horizon(1, gamma) raises for gamma == 1 (int(nan): ValueError) and gamma == 0 (1 / 0:
        # ZeroDivisionError); checked here, before the C loop sees a NaN horizon.  (Not in `allocation`: MCTS calls that,
        # and its errors stay as they were.)
        self.horizon(1, self.config["gamma"])
        self.config["episodes"], self.config["horizon"] = self.allocation(budget, self.config["gamma"])

    @staticmethod
    def allocation(budget, gamma):
        """Largest number of episodes e with e * horizon(e) <= budget, and that horizon (olop.py:50-62)."""
        return native.olop_allocation(budget, gamma)

    @staticmethod
    def value_upper_init(gamma, horizon):
        """A new node's value_upper by depth 0..horizon (olop.py:113), in Python arithmetic."""
        out = np.empty(int(horizon) + 1, np.float64)
        for depth in range(int(horizon) + 1):
            out[depth] = (1 - gamma ** (horizon + 1 - depth)) / (1 - gamma)
        return out

    def thresholds(self):
        """The bound's threshold for every episode (olop.py:145-158): the config string evaluated with ``time`` = the
        number of episodes ("global") or episode + 1 ("local")."""
        bound = self.config["upper_bound"]
        episodes = int(self.config["episodes"])
        out = np.zeros(episodes, np.float64)
        for episode in range(episodes):
            time = {"global": self.config["episodes"], "local": episode + 1}.get(bound["time"], np.nan)
            out[episode] = float(eval(bound["threshold"], {"np": np}, {"time": time}))
        return out

    # OLOP itself plans on deterministic tables and refuses anything else with the base class's TypeError, as it always has;
    # StochasticOLOP, below, sets this and plans on every finite MDP
    accepts_stochastic_models = False

    def model_for(self, state):
        """A deterministic table goes through the base class, and so does everything else unless the planner
        ``accepts_stochastic_models``.  Then a ``stochastic`` [S, A, S] or ``sparse`` [S, A, B] model is loaded with the env's
        availability table, its columns in the env's listing order (the expansion asks the clone which actions it lists,
        olop.py:169), and with the env's done rule (no step limit: done = terminated)."""
        mdp = None
        if self.accepts_stochastic_models and not device_model.is_cartpole(state):
            mdp = device_model.finite_mdp_of(state)
        if mdp is None or mdp.mode == "deterministic":
            return super(OLOP, self).model_for(state)
        available, order = device_model.availability_of(state, mdp)
        spec = device_model.spec_from_mdp(mdp, available=available, action_order=order)
        model = self.models.get(spec)
        if spec.available is not None and getattr(model, "available", None) is None:
            model.set_available(spec.available)          # (columns = listing order; as SparseSampling.model_for)
        model.set_episode_rules(getattr(mdp, "done_rule", "source"), 0)
        return model

    per_episode_kind = "olop"
    draws_survive_errors = True

    def plan_on(self, model, root_states, root_steps, rng_states, model_index=None, max_plan_len=None):
        """``root_steps`` is accepted for the common interface: the step limit ends no OLOP episode (done = terminated)."""
        cfg = self.config
        episodes, horizon = int(cfg["episodes"]), int(cfg["horizon"])        # KeyError without "episodes" (olop.py:95)
        kl = cfg["upper_bound"]["type"] == "kullback-leibler"
        if kl:
            if cfg["upper_bound"]["time"] not in ("global", "local"):
                logger.error("Unknown upper-bound time reference")
            thresholds = self.thresholds()
        else:
            logger.error("Unknown upper-bound type")
            thresholds = np.zeros(0, np.float64)
        # "uniform": a random new child; anything else: action 0 of the environment, in the device's labels
        continuation = -1 if cfg["continuation_type"] == "uniform" else int(self.device_actions([0], model)[0])
        args = (model, root_states, episodes, horizon, cfg["gamma"], kl, continuation, thresholds, self._value_upper_init, rng_states)
        if model.mode in (native.MODE_STOCHASTIC, native.MODE_SPARSE):
            # a dense / sparse model: the episodes sample it with the clone's generator (one model for every root)
            return self.models.ctx.olop_plan_stochastic(*args, max_plan_len=max_plan_len)
        return self.models.ctx.olop_plan(*args, max_plan_len=max_plan_len, model_index=model_index)

    @staticmethod
    def raise_for_status(status):
        status = np.asarray(status)
        failed = np.flatnonzero(status != native.MP_OK)
        if failed.size:
            if status[failed[0]] == native.ERR_OLOP_KEY:
                raise KeyError(0)                                                           # olop.py:89
            raise ValueError("This planner assumes that all rewards are normalized in [0, 1]")  # olop.py:133-134

    def plan_batch(self, state, root_states, root_steps=None, rng_states=None, env_rng_states=None):
        """``env_rng_states`` (what BatchedEvaluation hands every planner on a stochastic env) is accepted and ignored: every
        episode's clone is re-seeded with a draw of the planner's generator, so the environment's own is never read."""
        if "episodes" not in self.config:    # (olop.py:95; raised here, before anything is uploaded)
            raise KeyError("episodes")
        horizon = int(self.config["horizon"])
        model = self.model_for(state)
        self.about_to_plan()
        if rng_states is None:
            rng_states = self.batch_rng_states(len(root_states))
        out = self.plan_on(model, root_states, root_steps, rng_states, max_plan_len=max(horizon, 1))
        # the reference's observations and generator draws up to the failing step are taken before it raises: the step
        # count is booked, and the records in `rng_states` are advanced, also on an error
        self.env_steps += int(out["env_steps"].sum())
        self.raise_for_result(out)
        out["rng_states"] = rng_states
        self.relabel(out, model)
        self.last, self._root, self._last_model, self._last_actions = out, None, model, model.A
        self._last_stochastic = model.mode in (native.MODE_STOCHASTIC, native.MODE_SPARSE)
        self.claim_device_tree()
        return out

    def export_tree(self, root=0):
        self.require_device_tree()
        cfg = self.config
        cap = 1 + int(cfg["episodes"]) * int(cfg["horizon"]) * self._last_actions
        arrays = self.relabel_tree(self.models.ctx.olop_tree(root, cap), self._last_model)
        return build_olop_tree(arrays, self)

    def get_visits(self):
        """Observations stepped through (abstract.py:163-167).  On a deterministic model a node stands for one state and
        was stepped into ``count`` times, so the counts come from the exported tree (the last plan, as for OPD)."""
        from collections import defaultdict
        if self.last is not None and getattr(self, "_last_stochastic", False):
            raise NotImplementedError("on a stochastic model a node of the OLOP tree is an action sequence reached in many "
                                      "states and stands for no single one: the states stepped through leave no trace on "
                                      "the device and get_visits is not available")
        visits = defaultdict(int)
        if self.root is not None:
            for node, _ in self.root.breadth_first_search(self.root):
                if node.parent is not None and node.count > 0:
                    visits[str(node.state)] += node.count
        return visits


class OLOPNode(Node):
    """A node of an exported OLOP tree (olop.py:102-193): ``count``, ``cumulative_reward``, ``mu_ucb``, ``value_upper``,
    ``done``, ``state``."""
    STOP_ON_ANY_TERMINAL_STATE = False

    def get_value(self):
        return self.value_upper

    def selection_rule(self):
        """olop.py:126-130: the most visited children; among them the first whose value_upper nothing later exceeds."""
        labels = list(self.children)
        visits = [self.children[a].count for a in labels]
        most = max(visits)
        best = None
        for a, c in zip(labels, visits):
            if c == most and (best is None or self.children[a].value_upper > self.children[best].value_upper):
                best = a
        return best


def build_olop_tree(arrays, planner=None):
    """Creation-order arrays of mp_olop_tree_export -> linked :class:`OLOPNode` objects (children in creation order)."""
    nodes = []
    for i in range(len(arrays["parent"])):
        par = nodes[arrays["parent"][i]] if arrays["parent"][i] >= 0 else None
        node = OLOPNode(par, int(arrays["action"][i]), int(arrays["count"][i]), float(arrays["vu"][i]),
                        int(arrays["depth"][i]), planner)
        node.value_upper = float(arrays["vu"][i])
        node.mu_ucb = float(arrays["mu"][i])
        node.cumulative_reward = float(arrays["cum"][i])
        node.done = bool(arrays["done"][i])
        # (a stochastic model's export holds -1 below the root: such a node stands for no single state)
        node.state = int(arrays["state"][i]) if arrays["state"][i] >= 0 else None
        if par is not None:
            par.children[node.action] = node
        nodes.append(node)
    return nodes[0]


class OLOPAgent(AbstractTreeSearchAgent):
    """Drop-in for ``rl_agents.agents.tree_search.olop.OLOPAgent`` on deterministic finite-MDP tables; any other model is
    refused with ``TypeError``."""
    PLANNER_TYPE = OLOP


class StochasticOLOP(OLOP):
    """OLOP on every finite MDP: what :class:`OLOP` does on a deterministic table, and on a ``stochastic`` / ``sparse`` model
    the reference's own behaviour there (``mp_olop_plan_stochastic``): the clone re-seeded per episode, the state carried by
    the episode, a node's children fixed at its first expansion, ``done`` sticky per node."""
    accepts_stochastic_models = True


class StochasticOLOPAgent(AbstractTreeSearchAgent):
    """``rl_agents.agents.tree_search.olop.OLOPAgent`` with the reference's reach: the reference's OLOP / KL-OLOP configs
    (``SailingEnv/agents/kl-olop.json``) run on a ``StochasticMDP`` / ``SparseMDP`` env with only the ``__class__`` line
    changed.  :class:`OLOPAgent` keeps its name and its refusal of such envs, which earlier code may rely on."""
    PLANNER_TYPE = StochasticOLOP
