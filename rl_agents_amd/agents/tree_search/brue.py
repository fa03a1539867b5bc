"""Best Recommendation with Uniform Exploration, BRUE, on the MI355X planning core (reference
``rl_agents/agents/tree_search/brue.py``); the rollouts run in ``mp_brue_plan`` (rl_agents_amd/csrc/brue.hip).

Same class names, config keys and results as the reference on deterministic, ``stochastic`` and ``sparse`` finite-MDP
tables: the closed-loop planner for stochastic models.  The host computes the budget split (``OLOP.allocate_budget``) and
the table of ``gamma ** d`` (Python ``**``); everything else -- the rollouts with the clone re-seeded per rollout, the
running means, the nested ``estimate`` descents, the root's tie-break -- is the device's, bit for bit.
"""
import logging

import numpy as np

from rl_agents_amd import device_model
from rl_agents_amd.agents.tree_search.abstract import AbstractTreeSearchAgent, Node
from rl_agents_amd.agents.tree_search.olop import OLOP

logger = logging.getLogger(__name__)


class BRUE(OLOP):
    """BRUE planner (brue.py:11-75) for one or many roots of one finite MDP."""

    def reset(self):
        """brue.py:19-22.  Without "horizon" in the config the budget is split as OLOP does (``episodes`` is not used)."""
        super(OLOP, self).reset()
        if self.config["step_strategy"] == "subtree":
            # the reference makes a ChanceNode the root (abstract.py:201-203) and fails in update, which asks it for the
            # chance child of an action (brue.py:41)
            raise NotImplementedError("step_strategy 'subtree' is not available for BRUE")
        if "horizon" not in self.config:
            self.allocate_budget()

    @staticmethod
    def gamma_powers(gamma, horizon):
        """gamma ** d for d = 0..horizon in Python arithmetic (brue.py:63)."""
        return np.asarray([gamma ** d for d in range(int(horizon) + 1)], np.float64)

    def model_for(self, state):
        """Any finite MDP: deterministic tables, ``stochastic`` [S, A, S] and ``sparse`` [S, A, B] models.  BRUE draws its
        actions uniformly over ALL of them (brue.py:27) and never asks the environment which are available or in what
        order it lists them: the model is loaded without either."""
        mdp = device_model.finite_mdp_of(state)
        model = self.models.get(device_model.spec_from_mdp(mdp))
        if mdp.mode != "deterministic":
            model.set_episode_rules(getattr(mdp, "done_rule", "source"), 0)
        return model

    per_episode_kind = "brue"

    def plan_on(self, model, root_states, root_steps, rng_states, model_index=None, max_plan_len=None):
        """``root_steps`` and ``max_plan_len`` are accepted for the common interface: the step limit ends no BRUE rollout (done
        = terminated) and a plan is ONE action -- ``plans`` [n, 1], -1 where no rollout was made."""
        cfg = self.config
        horizon = int(cfg["horizon"])
        out = self.models.ctx.brue_plan(model, root_states, int(cfg["budget"]), horizon, cfg["gamma"],
                                        self.gamma_powers(cfg["gamma"], horizon), rng_states, model_index=model_index)
        n = len(out["plans"])
        out["plans"], out["plan_len"] = out["plans"].reshape(n, 1), np.ones(n, np.int32)
        return out

    def raise_for_result(self, out):
        if (out["plans"] < 0).any():
            # no rollout was made (budget <= 0): the reference's np.amax([]) of the root's selection raises (brue.py:75)
            raise ValueError("zero-size array to reduction operation maximum which has no identity")

    def plan_batch(self, state, root_states, root_steps=None, rng_states=None, env_rng_states=None):
        """``env_rng_states`` (what BatchedEvaluation hands every planner on a stochastic env) is accepted and ignored: every
        episode's clone is re-seeded with a draw of the planner's generator, so the environment's own is never read."""
        model = self.model_for(state)
        self.about_to_plan()
        if rng_states is None:
            rng_states = self.batch_rng_states(len(root_states))
        out = self.plan_on(model, root_states, root_steps, rng_states)
        self.env_steps += int(out["env_steps"].sum())
        out["rng_states"] = rng_states
        self._cap = 1 + 2 * (max(int(self.config["budget"]), 0) + int(self.config["horizon"]))
        self.last, self._root, self._last_model = out, None, model
        self.claim_device_tree()
        self.raise_for_result(out)          # (after the draws, the steps and the tree of the failing plan are booked)
        return out

    def export_tree(self, root=0):
        self.require_device_tree()
        return build_brue_tree(self.models.ctx.brue_tree(root, self._cap), self)

    def get_visits(self):
        """Observations stepped through (abstract.py:163-167): every model step leads to a decision node and counts once
        there, so the counts come from the exported tree's decision nodes by their observation (the last plan)."""
        from collections import defaultdict
        visits = defaultdict(int)
        if self.root is not None:
            for node, _ in self.root.breadth_first_search(self.root):
                if isinstance(node, DecisionNode) and node.parent is not None and node.count > 0:
                    visits[str(node.observation)] += node.count
        return visits


class DecisionNode(Node):
    """A state node of an exported BRUE tree (brue.py:78-96): ``count``, ``reward`` (the running mean of R(s, a, s')),
    ``children`` by action in creation order, ``observation`` (the state; None at the root)."""

    def get_value(self):
        return self.reward

    def selection_rule(self):
        """brue.py:88-91 without the tie draw: the first maximum (a viewer must not consume the planner's stream)."""
        if not self.children:
            return None
        return max(self.children, key=lambda a: self.children[a].value)


class ChanceNode(Node):
    """An action node of an exported BRUE tree (brue.py:99-116): ``count``, ``value`` (the running mean of the estimated
    returns), ``children`` by ``str(observation)`` in creation order."""

    def selection_rule(self):
        raise AttributeError("Selection is done in DecisionNodes, not ChanceNodes")


def build_brue_tree(arrays, planner=None):
    """Creation-order arrays of mp_brue_tree_export -> linked :class:`DecisionNode` / :class:`ChanceNode` objects."""
    nodes = []
    for i in range(len(arrays["parent"])):
        par = nodes[arrays["parent"][i]] if arrays["parent"][i] >= 0 else None
        key, stat = int(arrays["key"][i]), float(arrays["stat"][i])
        if arrays["is_chance"][i]:
            node = ChanceNode(par, key, int(arrays["count"][i]), stat, int(arrays["depth"][i]), planner)
            par.children[key] = node
        else:
            node = DecisionNode(par, None if par is None else str(key), int(arrays["count"][i]), stat,
                                int(arrays["depth"][i]), planner)
            node.reward = stat
            node.observation = None if par is None else key
            if par is not None:
                par.children[str(key)] = node
        nodes.append(node)
    return nodes[0]


class BRUEAgent(AbstractTreeSearchAgent):
    """Drop-in for ``rl_agents.agents.tree_search.brue.BRUEAgent``."""
    PLANNER_TYPE = BRUE
