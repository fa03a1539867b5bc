"""Sparse Sampling (Kearns, Mansour, Ng) on the MI355X planning core (reference
``rl_agents/agents/tree_search/sparse_sampling.py``); the recursion runs in ``mp_ss_plan``
(rl_agents_amd/csrc/sparse_sampling.hip).

Same class names, config keys and results as the reference on deterministic, ``stochastic`` and ``sparse`` finite-MDP
tables.  ``"horizon"`` and ``"C"`` have no default (``KeyError`` at plan time, as in the reference); ``budget`` plays no
part.  The samples step a clone directly (sparse_sampling.py:81), not through ``planner.step``: the reference's own step
count stays 0 and so does ``env_steps`` here; the model steps taken are counted in ``samples``.  Everything a plan computes
-- the draws, the clones' seeding, the outcome lists, the backups, the root's tie-break -- is the device's, bit for bit
(DESIGN.md).

One model per episode: ``SparseSampling.plan_on(..., model_index=...)`` plans every root on its own deterministic table of a batch
model (``mp_ss_plan_models``).  ``PerEpisodeEvaluation`` refuses the agent unasked, as it always has (``per_episode_kind = None``),
and runs it on request: ``PerEpisodeEvaluation(envs, agent, kind="ss")`` (``per_episode_kind_on_request``).
"""
import logging
from collections import defaultdict

import numpy as np

from rl_agents_amd import device_model, native
from rl_agents_amd.agents.tree_search.abstract import AbstractPlanner, AbstractTreeSearchAgent, Node

logger = logging.getLogger(__name__)


class SparseSampling(AbstractPlanner):
    """Sparse Sampling planner (sparse_sampling.py:11-28) for one or many roots of one finite MDP."""
    # PerEpisodeEvaluation refuses this planner by default (earlier code relies on the refusal); asked for by name,
    # PerEpisodeEvaluation(..., kind="ss"), it plans on one MDP per root (Context.ss_plan with model_index, mp_ss_plan_models)
    per_episode_kind = None
    per_episode_kind_on_request = "ss"

    def __init__(self, env, config=None):
        self.env = env
        self.samples = 0            # model steps of every plan so far (the reference keeps no such count)
        super(SparseSampling, self).__init__(config)

    def reset(self):
        """sparse_sampling.py:18-19."""
        super(SparseSampling, self).reset()
        if self.config["step_strategy"] == "subtree":
            # the reference makes a ChanceNode the root (abstract.py:201-203) and fails in plan, which asks it for
            # estimateV (sparse_sampling.py:22)
            raise NotImplementedError("step_strategy 'subtree' is not available for Sparse Sampling")

    def model_for(self, state):
        """Any finite MDP: deterministic tables, ``stochastic`` [S, A, S] and ``sparse`` [S, A, B] models.  This planner
        asks the environment which actions it lists (sparse_sampling.py:40-43): the model is loaded with the env's
        availability table, its columns in the env's listing order."""
        mdp = device_model.finite_mdp_of(state)
        available, order = device_model.availability_of(state, mdp)
        spec = device_model.spec_from_mdp(mdp, available=available, action_order=order)
        model = self.models.get(spec)
        if spec.available is not None and getattr(model, "available", None) is None:
            # a table model got the flags at its upload; a dense / sparse one gets them here, once, and not in the model cache:
            # MCTS plans on the same kinds of model and reads availability through its policies, never from the model
            model.set_available(spec.available)          # (columns = listing order)
        return model

    def plan_sizes(self):
        """(horizon, C) of the config, with what the reference raises for them at plan time."""
        cfg = self.config
        horizon = cfg["horizon"]                                     # KeyError: neither has a default
        if horizon == 0:
            # the root gets no child (:45-46): np.amax([]) of the root's selection raises (:55, abstract.py:301)
            raise ValueError("zero-size array to reduction operation maximum which has no identity")
        n_samples = cfg["C"]
        if n_samples < 1:
            # (the reference's UnboundLocalError: its backup reads the reward of a sample that was never taken, :87)
            raise ValueError("Sparse Sampling needs C >= 1 samples per chance node, got {}".format(n_samples))
        return int(horizon), int(n_samples)

    def plan_on(self, model, root_states, root_steps, rng_states, model_index=None, max_plan_len=None):
        """The one ``ctx.ss_plan`` call -> the binding's dict with ``plans`` [n, 1], ``plan_len`` and ``env_steps`` added.
        ``root_steps`` is accepted for the common interface: ``done`` is never read (sparse_sampling.py:81).  ``model_index``:
        a batch model, one MDP per root (mp_ss_plan_models).  ``max_plan_len``: a plan is one action whatever is asked for."""
        horizon, n_samples = self.plan_sizes()
        n = len(root_states)
        out = self.models.ctx.ss_plan(model, root_states, horizon, n_samples, self.config["gamma"], rng_states,
                                      model_index=model_index)
        self.samples += int(out["samples"].sum())
        out["env_steps"] = np.zeros(n, np.int64)                     # len(planner.observations): planner.step is not used
        out["plans"] = out["plans"].reshape(n, 1)
        out["plan_len"] = np.ones(n, np.int32)
        return out

    def raise_for_result(self, out):
        if (out["status"] != 0).any():
            raise RuntimeError("Sparse Sampling: the device refused a root (status {})".format(
                int(out["status"][out["status"] != 0][0])))

    def plan_batch(self, state, root_states, root_steps=None, rng_states=None, env_rng_states=None):
        """``root_steps`` and ``env_rng_states`` are accepted for the common interface: ``done`` is never read
        (sparse_sampling.py:81), and a clone is seeded anew before its one step (:79), whatever generator it copied."""
        self.plan_sizes()
        n = len(root_states)
        model = self.model_for(state)
        self.about_to_plan()
        if rng_states is None:
            rng_states = self.batch_rng_states(n)
        out = self.plan_on(model, root_states, root_steps, rng_states)
        out["rng_states"] = rng_states
        self.relabel(out, model)
        self.last, self._root, self._last_model = out, None, model
        self.claim_device_tree()
        self.raise_for_result(out)
        return out

    def plan(self, state, observation):
        """SparseSampling.plan (sparse_sampling.py:21-24), with the planner's generator written back also when the plan
        raises."""
        s0, steps0 = device_model.env_root_state(state)
        rng = native.rng_state_from_generator(self.np_random).reshape(1, 6)
        try:
            out = self.plan_batch(state, [s0], [steps0], rng_states=rng)
        finally:
            native.generator_set_state(self.np_random, rng[0])
        return [int(out["plans"][0, 0])]

    def tree_arrays(self, root=0):
        """Creation-order arrays of a root's tree (mp_ss_tree_export), chance keys as the environment's action ids."""
        self.require_device_tree()
        arrays = self.models.ctx.ss_tree(root)
        order = self.action_order(self._last_model)
        if order is not None:
            key, chance = arrays["key"], arrays["is_chance"].astype(bool)
            arrays["key"] = np.where(chance, order[np.where(chance, key, 0)], key).astype(key.dtype)
        return arrays

    def export_tree(self, root=0):
        return build_ss_tree(self.tree_arrays(root), self)

    def get_visits(self):
        """abstract.py:163-167 over ``planner.observations``, which the samples never reach: empty."""
        return defaultdict(int)


class DecisionNode(Node):
    """A state node of an exported tree (sparse_sampling.py:31-61): ``count`` (samples that led here), ``value`` (0 at depth
    ``horizon``), ``children`` by action in listing order, ``observation`` (the state; None at the root)."""

    def selection_rule(self):
        """sparse_sampling.py:53-56 without the tie draw: the first maximum (a viewer must not consume the planner's
        stream)."""
        if not self.children:
            return None
        return max(self.children, key=lambda a: self.children[a].value)


class ChanceNode(Node):
    """An action node of an exported tree (sparse_sampling.py:64-96): ``value``, ``children`` by ``str(observation)`` in
    creation order."""

    def selection_rule(self):
        raise AttributeError("Selection is done in DecisionNodes, not ChanceNodes")


def build_ss_tree(arrays, planner=None):
    """Creation-order arrays of mp_ss_tree_export -> linked :class:`DecisionNode` / :class:`ChanceNode` objects."""
    nodes = []
    for i in range(len(arrays["parent"])):
        par = nodes[arrays["parent"][i]] if arrays["parent"][i] >= 0 else None
        key, value = int(arrays["key"][i]), float(arrays["value"][i])
        if arrays["is_chance"][i]:
            node = ChanceNode(par, key, 0, value, int(arrays["depth"][i]), planner)
            par.children[key] = node
        else:
            node = DecisionNode(par, None if par is None else str(key), int(arrays["count"][i]), value,
                                int(arrays["depth"][i]), planner)
            node.observation = None if par is None else key
            if par is not None:
                par.children[str(key)] = node
        nodes.append(node)
    return nodes[0]


class SparseSamplingAgent(AbstractTreeSearchAgent):
    """Drop-in for ``rl_agents.agents.tree_search.sparse_sampling.SparseSamplingAgent``."""
    PLANNER_TYPE = SparseSampling
