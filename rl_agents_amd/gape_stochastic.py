"""MDP-GapE with the reference's reach: ``max_next_states_count`` 1..32 on deterministic tables and on ``stochastic`` /
``sparse`` models (``mp_gape_plan_stochastic``, rl_agents_amd/csrc/gape_stoch.hip).

``StochasticMDPGapE(MDPGapE)`` adds the transition thresholds by count, the plan call with K placeholders per chance node and
the export of the tree in the reference's dict order; ``StochasticMDPGapEAgent(MDPGapEAgent)`` is the agent that plans with it.
Both are served by name from ``rl_agents_amd.agents.tree_search.mdp_gape``, which is where an agent config names them::

    "<class 'rl_agents_amd.agents.tree_search.mdp_gape.StochasticMDPGapEAgent'>"

They are defined in this module rather than in that one because the planner classes that modules of ``rl_agents_amd/agents``
define form a closed table with what ``PerEpisodeEvaluation`` does with each; this planner inherits ``per_episode_kind = None``
from ``MDPGapE`` and is refused there as ``MDPGapE`` is.
"""
import numpy as np

from rl_agents_amd import native
from rl_agents_amd.agents.tree_search.mdp_gape import ChanceNode, DecisionNode, MDPGapE, MDPGapEAgent

PLACEHOLDERS_MESSAGE = ("No more placeholder nodes available, we observed more next states than the 'max_next_states_count' "
                        "config")                                                              # mdp_gape.py:284-285


class StochasticMDPGapE(MDPGapE):
    """MDP-GapE with the reference's reach: ``max_next_states_count`` 1..32 on deterministic tables and on ``stochastic`` /
    ``sparse`` models (``mp_gape_plan_stochastic``, csrc/gape_stoch.hip).  A chance node holds that many placeholder children
    and its values come from the KL region around the next-state frequencies (``max_expectation_under_constraint``).
    :class:`MDPGapE` keeps its name and its refusals, which earlier code may rely on.

    Refused: ``max_next_states_count`` above 32 (NotImplementedError) or below 1 (ValueError), ``step_strategy: "subtree"``,
    a bound type other than ``"kullback-leibler"``, one model per episode (``per_episode_kind`` None), CartPole models."""

    per_episode_kind_on_request = None        # mp_gape_plan_stochastic takes no batch model: refused also when asked for
    accepts_stochastic_models = True          # OLOP.model_for: availability in listing order, the env's done rule
    MAX_NEXT_STATES = 32                      # a chance node's children fill half a wavefront

    def transition_thresholds(self):
        """``transition_threshold()`` by the count of a chance node, 1 .. episodes + 2 (mdp_gape.py:307-313): the config string
        ``upper_bound["transition_threshold"]`` evaluated with the reference's variable names; the device divides by the
        count.  (The reference's own JSON files spell the key ``threshold_transition``, which nothing reads: the default string
        stays after the config merge.)  What the ``eval`` raises is raised as it is."""
        bound = self.config["upper_bound"]
        names = dict(horizon=self.config["horizon"], actions=self.env.action_space.n, confidence=self.config["confidence"],
                     time=self.config["episodes"])
        counts = int(self.config["episodes"]) + 2
        out = np.zeros(counts, np.float64)
        for count in range(1, counts + 1):
            out[count - 1] = float(eval(bound["transition_threshold"], {"np": np}, dict(names, count=count)))
        return out

    def plan_batch(self, state, root_states, root_steps=None, rng_states=None, env_rng_states=None):
        """``root_steps`` is accepted for the common interface: the step limit ends no episode (done = terminated).
        ``env_rng_states`` (what BatchedEvaluation hands every planner on a stochastic env) is accepted and ignored: every
        episode's clone is re-seeded with a draw of the planner's generator, so the environment's own is never read."""
        cfg = self.config
        episodes, horizon, count = int(cfg["episodes"]), int(cfg["horizon"]), cfg["max_next_states_count"]
        if count != int(count) or int(count) < 1:
            raise ValueError("max_next_states_count {}: a chance node needs a placeholder for its first next state".format(count))
        if count > self.MAX_NEXT_STATES:
            raise NotImplementedError("max_next_states_count {} > {}: a chance node's children fill half a wavefront on the "
                                      "device".format(count, self.MAX_NEXT_STATES))
        if cfg["upper_bound"]["type"] != "kullback-leibler":
            raise ValueError("MDP-GapE needs the 'kullback-leibler' bound: with '{}' the reference only logs an error and "
                             "plans on infinite bounds".format(cfg["upper_bound"]["type"]))
        model = self.model_for(state)
        self.about_to_plan()
        n = len(root_states)
        if rng_states is None:
            rng_states = self.batch_rng_states(n)
        try:
            thresholds = self.thresholds()
        except Exception:
            # the reference evaluates the string at the first node update: one draw of the planner's generator and one model
            # step of every plan have been made by then (mdp_gape.py:67, :82-87; the clone's draws are its own generator's)
            for i in range(n):
                gen = np.random.Generator(np.random.PCG64(0))
                native.generator_set_state(gen, rng_states[i])
                gen.integers(2 ** 30)
                rng_states[i] = native.rng_state_from_generator(gen)
            self.env_steps += n
            raise
        transition = self.transition_thresholds()        # (raised as it is, before the plan: the generator is not advanced)
        tables = dict(threshold=thresholds, transition_threshold=transition, initial_value=self._value_init)
        for name, table in tables.items():
            if not np.isfinite(table).all():
                raise ValueError("MDP-GapE: the {} table is not finite at index {}: the reference plans on the NaN bounds it "
                                 "makes".format(name, int(np.flatnonzero(~np.isfinite(table))[0])))
        if not (np.isfinite(cfg["gamma"]) and np.isfinite(cfg["accuracy"])):
            raise ValueError("MDP-GapE: gamma and accuracy must be finite")
        order = self.action_order(model)
        n_env = int(state.action_space.n)
        column = None
        if order is not None or n_env != model.A:
            column = np.full(n_env, -1, np.int32)
            listed = np.arange(model.A) if order is None else np.asarray(order)
            column[listed[listed < n_env]] = np.flatnonzero(listed < n_env)
        out = self.models.ctx.gape_plan_stochastic(model, root_states, episodes, horizon, int(count), cfg["gamma"],
                                                   cfg["accuracy"], cfg["continuation_type"] == "uniform", n_env, column,
                                                   thresholds, transition, self._value_init, rng_states)
        # the reference's steps and draws up to the failing step are taken before it raises
        self.env_steps += int(out["env_steps"].sum())
        failed = np.flatnonzero(out["status"] != native.MP_OK)
        if failed.size:
            status = out["status"][failed[0]]
            if status == native.ERR_GAPE_PLACEHOLDERS:
                raise ValueError(PLACEHOLDERS_MESSAGE)
            if status == native.ERR_GAPE_NO_CHALLENGER:
                raise ValueError("max() arg is an empty sequence")                              # mdp_gape.py:247
            if status == native.ERR_ARG:
                raise ValueError("'a' cannot be empty unless no samples are taken")             # abstract.py:310-311 on a NaN bound
            raise ValueError("This planner assumes that all rewards are normalized in [0, 1]")  # olop.py:133-134
        out["rng_states"] = rng_states
        self.relabel(out, model)
        if order is not None:
            arms = out["best_challenger"]
            out["best_challenger"] = np.where(arms >= 0, order[np.maximum(arms, 0)], -1).astype(arms.dtype)
            for k, fill in (("child_lower", 0), ("child_upper", 0), ("child_count", -1)):
                back = np.full((n, max(n_env, int(order.max()) + 1)), fill, out[k].dtype)
                back[:, order] = out[k]
                out[k] = back
        self.budget_used = int(out["episodes_run"][0]) * horizon
        self.last, self._root, self._last_model = out, None, model
        self.claim_device_tree()
        return out

    def export_tree(self, root=0):
        """:class:`DecisionNode` / :class:`ChanceNode` objects of the last plan's tree, a chance node's children keyed and
        ordered as the reference's dict: ``"placeholder_i"`` for the placeholders left, then ``str(state)`` by first observation."""
        self.require_device_tree()
        arrays = self.models.ctx.gape_stoch_tree(root)
        order = self.action_order(self._last_model)
        if order is not None:
            act = arrays["action"]
            arrays["action"] = np.where(arrays["kind"] == 1, order[np.clip(act, 0, len(order) - 1)], act).astype(act.dtype)
        return build_gape_stoch_tree(arrays, self)


def build_gape_stoch_tree(arrays, planner=None):
    """Breadth-first arrays of mp_gape_stoch_tree_export (a parent before its children, children in dict order) -> linked
    :class:`DecisionNode` / :class:`ChanceNode` objects."""
    nodes = []
    for i in range(len(arrays["parent"])):
        par = nodes[arrays["parent"][i]] if arrays["parent"][i] >= 0 else None
        key, args = int(arrays["action"][i]), (int(arrays["count"][i]), float(arrays["vu"][i]), int(arrays["depth"][i]), planner)
        if arrays["kind"][i]:
            node = ChanceNode(par, key, *args)
            par.children[key] = node
        else:
            label = None if par is None else ("placeholder_{}".format(-1 - key) if key < 0 else str(key))
            node = DecisionNode(par, label, *args)
            node.cumulative_reward = float(arrays["cum"][i])
            node.mu_ucb, node.mu_lcb = float(arrays["mu_ucb"][i]), float(arrays["mu_lcb"][i])
            node.done = bool(arrays["done"][i])
            node.observation = None if par is None or key < 0 else key
            if par is not None:
                par.children[label] = node
        node.value_upper, node.value_lower = float(arrays["vu"][i]), float(arrays["vl"][i])
        node.state = int(arrays["state"][i])
        nodes.append(node)
    return nodes[0]

class StochasticMDPGapEAgent(MDPGapEAgent):
    """``rl_agents.agents.tree_search.mdp_gape.MDPGapEAgent`` with the reference's reach: its MDP-GapE configs with
    ``max_next_states_count: 2`` (``FiniteMDPEnv``, ``SailingEnv``, ``DummyEnv``) run on deterministic, ``stochastic`` and
    ``sparse`` finite-MDP envs with only the ``__class__`` line changed.  :class:`MDPGapEAgent` keeps its name and its refusals."""
    PLANNER_TYPE = StochasticMDPGapE
