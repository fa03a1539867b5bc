"""MCTS / UCT agent on the MI355X planning core (reference ``rl_agents/agents/tree_search/mcts.py``).

Same class names, config keys and results as the reference; the episodes run in ``mp_uct_plan``
(rl_agents_amd/csrc/uct.hip).  Deviations, all documented in DESIGN.md:
* ``horizon`` given without ``episodes``: the reference raises KeyError (mcts.py:116-118,180); here
  ``episodes = budget // horizon``.

``closed_loop=True`` (mcts.py:147, MCTSNode.get_child :267-273) inserts, under every action node, one child per
observation seen after that action.  The environments the device plans on are deterministic, so an action node only
ever sees ONE observation, and that observation node receives exactly the updates of its action node (both lie on
every path through either): the statistics, the generator stream and the actions of a closed-loop plan are those of
the open-loop plan, which is what the device computes; the observation layer -- ``str(observation)`` keys in
``plan()``'s result and in the exported tree, prior 0 -- is rebuilt on the host by replaying the actions on a copy of
the environment.  Pinned on reference runs with ``closed_loop: true`` (tests/golden/variants.npz).

Environments exposing ``get_available_actions`` (mcts.py:59-97): the policy configs become per-state tables over the
available actions plus the table of actions the prior policy lists (``mp_policy_load_listed``): children exist for
listed actions only and ``len(children)`` in the exploration term is their number.
"""
import copy
import logging

import numpy as np

from rl_agents_amd import device_model
from rl_agents_amd import native as native_modes
from rl_agents_amd.agents.tree_search.abstract import AbstractPlanner, AbstractTreeSearchAgent, build_tree
from rl_agents_amd.agents.tree_search.olop import OLOP

logger = logging.getLogger(__name__)


def policy_probabilities(policy_config, n_actions):
    """Action distribution of a prior / rollout policy config over actions 0..n-1 (mcts.py:33-97).

    ``random`` and ``random_available`` are uniform; ``preference`` makes ``action`` ``ratio`` times
    likelier than each other action (uniform if that action does not exist)."""
    kind = policy_config["type"]
    if kind in ("random", "random_available"):
        return np.ones(n_actions) / n_actions
    if kind == "preference":
        action, ratio = policy_config["action"], policy_config.get("ratio", 2)
        if 0 <= action < n_actions:
            p = np.ones(n_actions) / (n_actions - 1 + ratio)
            p[action] *= ratio
            return p
        return np.ones(n_actions) / n_actions
    raise ValueError("Unknown policy type")


def policy_tables(policy_config, available, col_ids=None, env_rank=None):
    """A prior / rollout policy config on an environment that restricts (or orders) its available actions -> (probabilities
    [S, A], listed bool [S, A], slots uint8 [S, A] or None).  ``available``: bool [S, A] in the DEVICE's column order;
    ``col_ids[j]``: the environment action id of column j (None: ascending); ``env_rank[e]``: the position of action e in
    the environment's own listing (None: ascending).

    Row s of the table is what the reference's policy function returns in state s (mcts.py:46-97), zero on the actions
    it does not list.  Arithmetic as there: ``ones(k) / k``, ``ones(k) / (k - 1 + ratio)`` then ``*= ratio`` on the
    preferred action.  ``slots[s]`` is the order in which the policy LISTS the columns -- ``random`` lists
    ``np.arange(n)`` whatever the environment lists, the other two list ``get_available_actions()`` -- and is None when
    that is the column order anyway (then the inverse CDF over columns is the reference's)."""
    available = np.asarray(available).astype(bool)
    n_states, n_actions = available.shape
    col_ids = np.arange(n_actions) if col_ids is None else np.asarray(col_ids, dtype=np.int64)
    env_rank = np.arange(n_actions) if env_rank is None else np.asarray(env_rank, dtype=np.int64)
    kind = policy_config["type"]
    if kind == "random":                                          # ignores availability (mcts.py:46-57)
        table, listed = np.ones((n_states, n_actions)) / n_actions, np.ones((n_states, n_actions), dtype=bool)
        key = np.broadcast_to(col_ids, (n_states, n_actions))                         # listed by ascending action id
    else:
        k = available.sum(axis=1)
        uniform = np.where(available, (np.ones(n_states) / k)[:, None], 0.0)
        listed = available
        if kind == "random_available":
            table = uniform
        elif kind == "preference":
            action, ratio = policy_config["action"], policy_config.get("ratio", 2)
            table = uniform
            if 0 <= action < n_actions:
                has = available[:, action]
                base = np.ones(n_states) / (k - 1 + ratio)
                pref = np.where(available, base[:, None], 0.0)
                pref[:, action] = np.where(has, base * ratio, 0.0)
                table = np.where(has[:, None], pref, uniform)
        else:
            raise ValueError("Unknown policy type")
        # listed in the environment's order, the unlisted columns after them
        key = np.where(available, env_rank[col_ids][None, :], n_actions + np.arange(n_actions)[None, :])
    slots = np.argsort(key, axis=1, kind="stable").astype(np.uint8)
    # the order only matters among the columns with a positive probability
    ascending = True
    for s_row, t_row in zip(slots, table > 0):
        cols = s_row[t_row[s_row]]
        if np.any(np.diff(cols.astype(np.int64)) < 0):
            ascending = False
            break
    return table, listed, (None if ascending else slots)


class MCTS(AbstractPlanner):
    """UCT planner (mcts.py:100-200) for one or many roots of one finite MDP (or closed-form CartPole)."""
    supports_cartpole = True
    per_episode_kind = "uct"

    def __init__(self, env, prior_policy, rollout_policy, config=None):
        super(MCTS, self).__init__(config)
        self.env = env
        self.prior_policy = prior_policy        # policy config dicts (resolved per model: needs |A|)
        self.rollout_policy = rollout_policy
        # per-state policies (mcts_with_prior.py): callable(state, model) -> (prior [S,A], rollout [S,A]), or None
        self.policy_source = None
        self._policies = {}
        if not self.config["horizon"]:
            self.config["episodes"], self.config["horizon"] = OLOP.allocation(self.config["budget"],
                                                                              self.config["gamma"])
        elif not self.config.get("episodes"):
            self.config["episodes"] = max(self.config["budget"] // self.config["horizon"], 1)
        self._closed_plan = None
        self._restricted = {}      # id(model) -> (model, prior, rollout, listed) tables of a restricted-action env

    @classmethod
    def default_config(cls):
        cfg = super(MCTS, cls).default_config()
        # the reference derives the default temperature from the DEFAULT gamma (0.8), whatever gamma
        # the user configures (mcts.py:121-124); kept
        cfg.update({"temperature": 2 / (1 - cfg["gamma"]), "closed_loop": False})
        return cfg

    def reset(self):
        super(MCTS, self).reset()
        self._armed = False         # the device holds kept trees armed for re-rooting by this planner
        self._tree_roots = 0        # number of roots of the trees this planner's last plan left on the device

    def step_by_subtree(self, action):
        """Tree reuse: the device re-roots the kept trees at the start of the next plan, provided the trees on the
        context are still this planner's (nothing else planned in between); otherwise the tree is reset."""
        if self.config["closed_loop"]:
            # the reference re-roots at the ACTION node, whose children are keyed by observation strings: its next
            # run() would step the environment with such a key (abstract.py:195-206 + mcts.py:143-146)
            raise NotImplementedError("step_strategy 'subtree' does not work on closed-loop trees (in the reference either)")
        # every act() steps the tree (abstract.py:70-82), also between two plans when receding_horizon > 1: the device
        # descends one level per call (a pending re-rooting is applied when the next one is armed)
        live = self.last is not None or self._armed
        # the kept trees must be ONE tree: after a multi-root plan_batch the reference's "action not in children" path
        # (abstract.py:200-206) is the nearest meaning -- start over (used to surface MP_ERR_ARG from act())
        if not live or not self.owns_device_tree() or self._tree_roots != 1:
            self.step_by_reset()
            return
        labels = self.device_actions([int(action)], getattr(self, "_last_model", None))
        self.models.ctx.uct_step_tree(labels)
        if not getattr(self, "_visit_gap", None):
            self._visit_events().append(("step", np.asarray(labels, dtype=np.int32).copy()))
        self.last, self._root = None, None
        self._armed = True

    # -- get_visits (abstract.py:163-167): rollouts leave no trace in the tree, so the single-root plans are logged (root
    # state, generator records, policies: a few hundred bytes each) and REPLAYED on demand with the visit counter armed
    # (mp_uct_record_visits) -- on a private context, so the trees of the real plans stay where they are.
    def _visit_events(self):
        if not hasattr(self, "_visit_log"):
            self._visit_log, self._visit_done, self._visit_counts = [], 0, {}
            self._visit_gap = None
            self._visit_roots = {}          # batch slot -> {state: count}: what N sequential planners would each answer
            self._visit_bytes = 0
        return self._visit_log

    def _device_clone(self, x):
        """A copy of a device tensor made on the planner's stream (where the loop that owns the tensor writes it)."""
        import torch
        with torch.cuda.stream(torch.cuda.ExternalStream(self.models.ctx.stream_ptr(), device=x.device)):
            return x.detach().clone()

    def reset_visits(self):
        """Forget the visit log, the counts and any gap (get_visits then counts the plans made from here on).  The
        reference's ``planner.observations`` is never cleared (abstract.py:114,160), so nothing calls this implicitly."""
        self._visit_log, self._visit_done, self._visit_counts = [], 0, {}
        self._visit_gap, self._visit_roots, self._visit_bytes = None, {}, 0

    def _log_plan(self, model, root_states, root_steps, rng_states, env_rng_states, policy, continued):
        """Called right BEFORE a plan: everything a replay needs (``policy``: ("tables", prior, rollout, listed, slots)
        or ("flat", prior_p, rollout_p))."""
        events = self._visit_events()
        if len(events) > 20000:     # nobody asked for visits in 20 000 plans: stop logging (a few MB), say so when asked
            del events[:]
            self._visit_gap = "more than 20 000 plans since get_visits was last asked: the log was dropped"
        if self._visit_gap:
            return
        n = len(root_states)
        if getattr(model, "spec", None) is None:
            self._visit_gap = "observations of this environment are not states of a finite MDP"
            return
        # a batched plan is logged like a single-root one -- 60 bytes per root (root, step count, generator records) -- up to
        # 512 MB of log since get_visits was last asked
        self._visit_bytes += 64 * n
        if self._visit_bytes > (512 << 20):
            del events[:]
            self._visit_gap = "more than 512 MB of batched plans since get_visits was last asked: the log was dropped"
            return
        rules = getattr(model, "episode_rules", None)    # stochastic / sparse models: set after the upload (model_for)
        cfg = self.config

        def host(x, dtype, shape):
            if x is None:
                return None
            if hasattr(x, "detach"):                     # a device tensor (device-resident loops with record_visits): a device-side
                import torch                             # copy now, ON THE PLANNER'S STREAM (the loop's env step writes these
                ctx = self.models.ctx                    # buffers there); brought to the host when replayed
                with torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream_ptr(), device=x.device)):
                    return x.detach().clone()
            return np.array(x, dtype=dtype).reshape(shape).copy()
        events.append(("plan", dict(
            spec=model.spec, rules=rules, n=n, s0=host(root_states, np.int32, n), steps0=host(root_steps, np.int32, n),
            rng=host(rng_states, np.uint64, (n, 6)), erng=host(env_rng_states, np.uint64, (n, 6)),
            episodes=cfg["episodes"], horizon=cfg["horizon"], gamma=cfg["gamma"], temperature=cfg["temperature"],
            closed=bool(cfg["closed_loop"]), policy=policy, continued=bool(continued))))

    def get_visits(self):
        """How often the planner's env steps -- descents and rollouts of every plan so far -- observed each state
        (``str(observation)`` -> count), as the reference's ever-growing ``planner.observations`` gives it.  Batched plans
        count for every root of the batch (the sum of what N sequential planners would answer: :meth:`get_visits_per_root`
        has them one by one)."""
        from collections import defaultdict
        self._replay_visits()
        out = defaultdict(int)
        for s, c in self._visit_counts.items():
            out[str(s)] = c
        return out

    def get_visits_per_root(self):
        """Batched plans: ``get_visits()`` of each batch slot -- what the planner of a sequential agent i would answer
        (abstract.py:163-167 for N planner objects) -- as a list of ``{str(state): count}`` indexed by slot."""
        from collections import defaultdict
        self._replay_visits()
        n = 1 + max(self._visit_roots) if self._visit_roots else 0
        out = []
        for i in range(n):
            d = defaultdict(int)
            for s, c in self._visit_roots.get(i, {}).items():
                d[str(s)] = c
            out.append(d)
        return out

    def _replay_visits(self):
        from rl_agents_amd import native
        events = self._visit_events()
        if self._visit_gap:
            raise NotImplementedError("get_visits: " + self._visit_gap)
        if self._visit_done >= len(events):
            return
        if not hasattr(self, "_replay_models"):
            self._replay_models = device_model.ModelCache(ctx=native.Context(self.models.ctx.device))
            self._replay_policies = {}
        cache, ctx = self._replay_models, self._replay_models.ctx

        def to_host(x, dtype):
            if x is None or isinstance(x, np.ndarray):
                return x
            arr = x.cpu().numpy()                         # (device clones of a device-resident loop)
            return arr.view(np.uint64) if dtype == np.uint64 else arr.astype(dtype)
        for kind, e in events[self._visit_done:]:
            if kind == "step":
                ctx.uct_step_tree(to_host(e, np.int32))
                continue
            model = cache.get(e["spec"])
            if e["rules"] is not None:
                model.set_episode_rules(*e["rules"])
            if not e["continued"]:
                ctx.uct_reset_tree()
            policy, pp, rp = None, None, None
            if e["policy"][0] == "tables":
                _, prior, rollout, listed, slots = e["policy"]
                key = (id(model), id(prior), id(rollout))
                hit = self._replay_policies.get(key)
                if hit is None:
                    hit = (prior, rollout, ctx.load_policy(model, prior, rollout, listed=listed, rollout_slots=slots))
                    self._replay_policies = {key: hit}         # (one at a time: a policy is tied to its model)
                policy = hit[2]
            else:
                _, pp, rp = e["policy"]
            n = e["n"]
            s0, steps0 = to_host(e["s0"], np.int32), to_host(e["steps0"], np.int32)
            rng, erng = to_host(e["rng"], np.uint64), to_host(e["erng"], np.uint64)
            # the whole batch in one launch when its [n, S] visit matrix stays under 256 MB, else chunk by chunk (a plan that
            # continues kept trees needs the whole batch's trees on the replay context: it is not chunked)
            chunk = max(1, min(n, (256 << 20) // (4 * model.S)))
            if e["continued"] and chunk < n:
                raise NotImplementedError("get_visits: a batched plan on kept subtrees of {} roots x {} states does not fit the "
                                          "replay buffer".format(n, model.S))
            for lo in range(0, n, chunk):
                hi = min(n, lo + chunk)
                visits = np.zeros((hi - lo, model.S), dtype=np.int32)
                ctx.uct_plan_stochastic(model, s0[lo:hi], e["episodes"], e["horizon"], e["gamma"], e["temperature"], pp, rp,
                                        np.ascontiguousarray(rng[lo:hi]).copy(),
                                        env_rng_state=None if erng is None else np.ascontiguousarray(erng[lo:hi]),
                                        closed_loop=e["closed"], root_steps=None if steps0 is None else steps0[lo:hi],
                                        policy=policy, visits=visits)
                rows, cols = np.nonzero(visits)
                for r_, c_ in zip(rows.tolist(), cols.tolist()):
                    k = int(visits[r_, c_])
                    self._visit_counts[c_] = self._visit_counts.get(c_, 0) + k
                    per = self._visit_roots.setdefault(lo + r_, {})
                    per[c_] = per.get(c_, 0) + k
        del events[:]                                  # replayed: only the counts are kept
        self._visit_done, self._visit_bytes = 0, 0

    def model_for(self, state):
        """Deterministic tables / CartPole as every planner; MCTS also plans on STOCHASTIC finite MDPs (`stochastic`,
        `sparse` modes: the reference's planner steps any env, tree_search/abstract.py:158-161)."""
        if not device_model.is_cartpole(state):
            mdp = device_model.finite_mdp_of(state)
            if mdp.mode in ("stochastic", "sparse"):
                # (columns in the PRIOR policy's listing order, as for the deterministic tables below)
                available, order = device_model.availability_of(state, mdp)
                self._env_order = order
                tree_order = None if self.prior_policy["type"] == "random" and self.policy_source is None else order
                spec = device_model.spec_from_mdp(mdp, available=available, action_order=tree_order)
                model = self.models.get(spec)
                model.episode_rules = (getattr(mdp, "done_rule", "source"), device_model.env_max_steps(state))
                model.set_episode_rules(*model.episode_rules)
                # (restrictions reach the kernel through the per-state policy tables, not through the model)
                model.available = None if spec.available is None else spec.available.astype(bool)
                return model
            if mdp.mode == "deterministic":
                # The columns of the device tables -- the order of a node's children and of every tie-break -- follow
                # the order in which the PRIOR policy lists the actions (mcts.py:237-246): the environment's listing
                # order, or np.arange(n) for policy type `random` (mcts.py:46-57), whatever the environment lists.
                available, order = device_model.availability_of(state, mdp)
                self._env_order = order
                tree_order = None if self.prior_policy["type"] == "random" and self.policy_source is None else order
                return self.models.get(device_model.spec_from_mdp(mdp, max_steps=device_model.env_max_steps(state),
                                                                  available=available, action_order=tree_order))
        return super(MCTS, self).model_for(state)

    def loop_form(self, model):
        """Per-state policies (restricted action sets, prior agents) over MORE THAN 8 ACTIONS on a deterministic table: the
        kernel of the stochastic models plans on deterministic ones too and has loop forms for any number of actions
        (uct.hip keeps a node's policy rows in registers: 2..8 actions).  Same planner, same results: the reference does
        not distinguish the two kinds of environment."""
        if model.mode != native_modes.MODE_DETERMINISTIC or model.A <= 8:
            return False
        if self.policy_source is None and getattr(model, "available", None) is None:
            return False
        return True

    def plan_batch_stochastic(self, state, model, root_states, root_steps, rng_states, env_rng_states=None):
        """The stochastic-model path (uct_stoch.hip): every root's episodes replay the noise of the ENV's generator as it
        is at plan time (clones copy it, common/factory.py:119-134); closed loop keys the tree by observed next states."""
        from rl_agents_amd import native
        n, cfg = len(root_states), self.config
        if env_rng_states is None and model.mode != native_modes.MODE_DETERMINISTIC:   # (a deterministic table draws nothing)
            gen = getattr(getattr(state, "unwrapped", state), "np_random", None)
            if gen is None:
                raise TypeError("a stochastic environment must expose its numpy generator as `np_random`")
            env_rng_states = np.tile(native.rng_state_from_generator(gen), (n, 1))
        policy, pp, rp, logged = self._policy_choice(state, model)
        self._log_plan(model, root_states, root_steps, rng_states, env_rng_states, logged, getattr(self, "_continued", False))
        out = self.models.ctx.uct_plan_stochastic(
            model, root_states, cfg["episodes"], cfg["horizon"], cfg["gamma"], cfg["temperature"], pp, rp, rng_states,
            env_rng_state=env_rng_states, closed_loop=cfg["closed_loop"], root_steps=root_steps, policy=policy)
        out["rng_states"] = rng_states
        order = self.action_order(model)
        if order is not None:           # device labels -> the environment's action ids (closed loop: every other entry is
            plans = out["plans"]        # an observation key)
            is_action = np.ones(plans.shape[1], dtype=bool)
            if cfg["closed_loop"]:
                is_action[1::2] = False
            out["plans"] = np.where((plans >= 0) & is_action[None, :], order[np.maximum(plans, 0) % len(order)], plans).astype(plans.dtype)
            for k in ("root_child_count", "root_child_value"):
                back = np.empty_like(out[k])
                back[:, order] = out[k]
                out[k] = back
        self._last_tables, self._last_model, self._stochastic = None, model, True
        self._stored_priors = policy is not None
        self.last, self._root, self._last_actions, self._last_env = out, None, model.A, state
        self._tree_roots = n
        self.claim_device_tree()
        self.env_steps += int(out["env_steps"].sum())
        return out

    def plan_batch(self, state, root_states, root_steps=None, rng_states=None, keep_actions=None, env_rng_states=None):
        self.about_to_plan()
        model = self.model_for(state)
        n = len(root_states)
        if rng_states is None:
            rng_states = self.batch_rng_states(n)
        if model.mode in (native_modes.MODE_STOCHASTIC, native_modes.MODE_SPARSE) or self.loop_form(model):
            self._continued = self._continue_trees(model, n, keep_actions, stochastic=True)
            return self.plan_batch_stochastic(state, model, root_states, root_steps, rng_states, env_rng_states)
        self._stochastic = False
        cfg = self.config
        continued = self._continue_trees(model, n, keep_actions, stochastic=False)
        policy, prior_p, rollout_p, logged = self._policy_choice(state, model)
        self._log_plan(model, root_states, root_steps, rng_states, None, logged, continued)
        out = self.models.ctx.uct_plan(model, root_states, cfg["episodes"], cfg["horizon"], cfg["gamma"], cfg["temperature"],
                                       prior_p, rollout_p, rng_states, root_steps=root_steps, max_plan_len=max(cfg["horizon"], 1),
                                       policy=policy)
        self._last_tables = None
        if policy is not None:
            order = self.action_order(model)
            prior_ids = prior = logged[1]
            if order is not None:                       # export works in the environment's action ids
                prior_ids = np.empty_like(prior)
                prior_ids[:, order] = prior
            self._last_tables = (np.asarray(device_model.finite_mdp_of(state).transition), prior_ids,
                                 np.asarray(root_states, dtype=np.int64))
        out["rng_states"] = rng_states
        self.relabel(out, model)
        self._last_model = model
        self.last, self._root, self._last_actions, self._last_env = out, None, model.A, state
        self._last_roots = np.asarray(root_states, dtype=np.int64) if model.mode == native_modes.MODE_DETERMINISTIC else None
        self._tree_roots = n
        self.claim_device_tree()
        self.env_steps += int(out["env_steps"].sum())
        return out

    # -- device-resident evaluation loop (BatchedEvaluation): roots, generator records and results are device buffers ----
    def supports_device_loop(self):
        """MCTS on deterministic tables: plain, with tree re-use (``step_strategy="subtree"``: the kept trees are re-rooted
        on the device from the action buffer) and closed loop (on a deterministic model the first action of a
        closed-loop plan is the open-loop plan's, see the module docstring)."""
        return True

    def device_plan_len(self, model):
        return 1

    def plan_batch_device(self, state, model, n, d_state, d_steps, d_rng, d_plans, d_len, d_env_steps, d_status, d_value=None,
                          keep_actions=None, d_env_rng=None):
        """One asynchronous batched plan (mp_uct_plan / mp_uct_plan_policy, MP_MEM_DEVICE): only enqueues.
        ``d_value``: optional float64 [n] buffer for the root values.  ``keep_actions``: contiguous int32 device tensor of
        the (device-label) actions executed since the last plan -- ``step_strategy="subtree"``: the trees of the last plan
        are re-rooted under them (abstract.py:195-206) instead of being reset."""
        cfg, ctx = self.config, self.models.ctx
        self.about_to_plan()
        self._visit_events()
        record = bool(cfg.get("record_visits"))      # opt-in: device-side copies of the roots / generator records of every step
        if not record:
            self._visit_gap = ("the plans of a device-resident evaluation loop are not logged (set the planner's config "
                               "'record_visits' to log them, or call reset_visits() afterwards)")
        # stochastic / sparse models (and the loop forms of deterministic ones): the kernel of the stochastic path; the episodes'
        # env generator records are a device buffer too (d_env_rng: every plan's clones start from the env generator as it is
        # at that step; mp_env_step_stochastic advances it)
        stochastic = model.mode != native_modes.MODE_DETERMINISTIC or self.loop_form(model)
        if stochastic and d_env_rng is None and model.mode != native_modes.MODE_DETERMINISTIC:
            raise ValueError("a stochastic model needs the episodes' env generator records (d_env_rng)")
        # the kept trees are stepped only where they are this planner's and as many as the roots (the stochastic path: open loop
        # only); the step event is logged under record_visits alone, as a device clone
        armed = keep_actions is not None and self.owns_device_tree() and self._tree_roots == n \
            and not (stochastic and cfg["closed_loop"])
        if armed:
            ctx.uct_step_tree(keep_actions)
            if record:
                self._visit_events().append(("step", self._device_clone(keep_actions)))
        else:
            ctx.uct_reset_tree()
        policy, pp, rp, logged = self._policy_choice(state, model)
        if record:
            self._log_plan(model, d_state[:n], None if d_steps is None else d_steps[:n], d_rng[:n],
                           d_env_rng[:n] if stochastic and d_env_rng is not None else None, logged, armed)
        if stochastic:
            ctx.uct_plan_stochastic_device(model, n, d_state, cfg["episodes"], cfg["horizon"], cfg["gamma"], cfg["temperature"], pp,
                                           rp, d_rng, d_env_rng, int(d_plans.shape[1]), closed_loop=cfg["closed_loop"],
                                           plans=d_plans, plan_len=d_len, root_value=d_value, env_steps=d_env_steps,
                                           root_steps=d_steps, policy=policy)
            self._stochastic = True
        else:
            ctx.uct_plan_device(model, n, d_state, cfg["episodes"], cfg["horizon"], cfg["gamma"], cfg["temperature"], pp, rp, d_rng,
                                int(d_plans.shape[1]), plans=d_plans, plan_len=d_len, root_value=d_value, env_steps=d_env_steps,
                                root_steps=d_steps, policy=policy)
        self.claim_device_tree()
        self.last, self._root, self._tree_roots = None, None, n

    def _policy_choice(self, state, model):
        """(device policy or None, prior_p, rollout_p, logged) of a plan on ``model``: flat policy vectors over the actions, or
        -- with a ``policy_source`` (a prior agent's distribution, mcts_with_prior.py:47-62) or an environment that restricts
        its actions (mcts.py:59-97) -- per-state [S, A] tables the kernel reads by the state the descent is in.  ``logged`` is
        what a replay needs (:meth:`_log_plan`): ("flat", prior_p, rollout_p) or ("tables", prior, rollout, listed, slots)."""
        available = getattr(model, "available", None)
        if self.policy_source is None and available is None:
            pp, rp = policy_probabilities(self.prior_policy, model.A), policy_probabilities(self.rollout_policy, model.A)
            return None, pp, rp, ("flat", pp, rp)
        if self.policy_source is not None:
            prior, rollout = self.policy_source(state, model)      # (restricted to the available actions there; columns in
            listed, slots = available, None                        #  the model's listing order)
        else:
            prior, rollout, listed, slots = self.restricted_policy_tables(model, available)
        return self.device_policy(model, prior, rollout, listed, slots), None, None, ("tables", prior, rollout, listed, slots)

    def _continue_trees(self, model, n, keep_actions, stochastic):
        """A host plan of ``n`` roots: the trees the last plan left are stepped by ``keep_actions`` (batched callers: the
        executed actions, environment ids), continued where :meth:`step_by_subtree` armed them, or reset -> whether the plan
        goes on in kept trees (logged for get_visits).  The stochastic path keeps open-loop trees only, and steps them only
        where they are as many as the roots; the deterministic path compares neither."""
        ctx, open_loop = self.models.ctx, not (stochastic and self.config["closed_loop"])
        armed, self._armed = self._armed and n == 1 and open_loop, False
        if keep_actions is not None and self.owns_device_tree() and open_loop and (not stochastic or self._tree_roots == n):
            labels = np.asarray(self.device_actions(keep_actions, model), dtype=np.int32)
            ctx.uct_step_tree(labels)
            if not getattr(self, "_visit_gap", None):
                self._visit_events().append(("step", labels.copy()))
        elif not (armed and self.owns_device_tree()):
            ctx.uct_reset_tree()
            return False
        return True

    def restricted_policy_tables(self, model, available):
        """(prior, rollout, listed, rollout slots) of this planner's policy configs on a model whose environment restricts
        or orders its actions, kept per model.  Columns are in the PRIOR policy's order (:meth:`model_for`); the rollout
        policy's own listing order comes back as ``slots`` when it differs (mp_policy_load_ordered)."""
        hit = self._restricted.get(id(model))
        if hit is None or hit[0] is not model:
            n = model.A
            order = self.action_order(model)
            col_ids = np.arange(n) if order is None else np.asarray(order, dtype=np.int64)
            env_order = getattr(self, "_env_order", None)
            env_rank = np.arange(n)
            if env_order is not None:
                env_rank = np.empty(n, dtype=np.int64)
                env_rank[np.asarray(env_order, dtype=np.int64)] = np.arange(n)

            def on_device(cfg):     # a preference policy names an environment action id: its column on the device
                if cfg.get("type") == "preference" and 0 <= cfg["action"] < n:
                    return dict(cfg, action=int(np.flatnonzero(col_ids == cfg["action"])[0]))
                return cfg
            prior, listed, prior_slots = policy_tables(on_device(self.prior_policy), available, col_ids, env_rank)
            assert prior_slots is None, "the device columns follow the prior policy's listing order"
            rollout, _, slots = policy_tables(on_device(self.rollout_policy), available, col_ids, env_rank)
            if len(self._restricted) >= 4:
                self._restricted.clear()
            hit = self._restricted[id(model)] = (model, prior, rollout, listed, slots)
        return hit[1], hit[2], hit[3], hit[4]

    def device_policy(self, model, prior, rollout, listed=None, slots=None):
        """Upload (once per model and table contents) the per-state policy tables."""
        # (model.epoch: a delta upload patched the model's tables -- the fused policy records hold the old transitions)
        key = (id(model), id(prior), id(rollout), getattr(model, "epoch", 0))
        hit = self._policies.get(key)
        if hit is None or hit[0] is not model or hit[1] is not prior or hit[2] is not rollout:
            if len(self._policies) >= 4:
                self._policies.clear()
            hit = (model, prior, rollout, self.models.ctx.load_policy(model, prior, rollout, listed=listed, rollout_slots=slots))
            self._policies[key] = hit
        return hit[3]

    # -- closed loop: the observation-keyed layer, rebuilt on the host (see the module docstring) ----------------
    def plan(self, state, observation):
        actions = super(MCTS, self).plan(state, observation)
        self._closed_plan = None
        if getattr(self, "_stochastic", False):
            if self.config["closed_loop"]:      # the device returns action, observation key, action, ...: keys are strings
                self._closed_plan = [a if i % 2 == 0 else str(a) for i, a in enumerate(actions)]
                return list(self._closed_plan)
            return actions
        if self.config["closed_loop"]:
            self._closed_plan = self._with_observation_keys(state, actions)
            return list(self._closed_plan)
        return actions

    def get_plan(self):
        if self.config["closed_loop"] and self._closed_plan is not None:
            return list(self._closed_plan)
        return super(MCTS, self).get_plan()

    def _with_observation_keys(self, state, actions):
        """[a0, a1, ...] -> [a0, str(obs1), a1, str(obs2), ...] as AbstractPlanner.get_plan walks a closed-loop tree
        (abstract.py:143-156): the key of an action node's child is the observation that followed the action; the last
        action is followed by one only if its node was visited (an unvisited action node has no child yet)."""
        if not actions:
            return []
        self.require_device_tree()
        # (one four-byte read-back of the last node's visit count: mp_uct_path_count -- not an export of the whole tree)
        model = getattr(self, "_last_model", None)
        last_visited = self.models.ctx.uct_path_count(0, self.device_actions(actions, model)) > 0
        env = copy.deepcopy(getattr(state, "unwrapped", state))     # never the live environment
        out = []
        for i, a in enumerate(actions):
            out.append(a)
            if i + 1 < len(actions) or last_visited:
                out.append(str(env.step(a)[0]))
        return out

    def export_tree(self, root=0):
        if getattr(self, "_stochastic", False):
            return self._export_stochastic(root)
        tree = self._export_open_loop(root)
        if self.config["closed_loop"]:
            self._insert_observation_nodes(tree, root)
        return tree

    def _export_stochastic(self, root=0):
        """Tree of a stochastic-model plan: action nodes keyed by action id (prior = the prior policy's probability),
        observation nodes keyed by str(next state) with prior 0 (mcts.py:267-273), children in dict order."""
        from rl_agents_amd.agents.tree_search.abstract import Node
        self.require_device_tree()
        t = self.models.ctx.uct_stoch_tree(root)
        order = self.action_order(getattr(self, "_last_model", None))
        if order is not None:           # action nodes' keys: device labels -> the environment's action ids
            act = t["action"]
            t["action"] = np.where((act >= 0) & (t["is_obs"] == 0), order[np.maximum(act, 0) % len(order)], act).astype(act.dtype)
        stored = getattr(self, "_stored_priors", False)     # per-state policies: the priors the device kept in the tree
        prior = None if stored else policy_probabilities(self.prior_policy, self._last_actions)
        nodes = []
        for i in range(len(t["parent"])):
            par = nodes[t["parent"][i]] if t["parent"][i] >= 0 else None
            obs = bool(t["is_obs"][i])
            key = None if par is None else (str(int(t["action"][i])) if obs else int(t["action"][i]))
            node = Node(par, key, int(t["count"][i]), float(t["value"][i]), 0 if par is None else par.depth + (0 if obs else 1))
            node.prior = 1.0 if par is None else (0 if obs else float(t["prior"][i] if stored else prior[int(t["action"][i])]))
            if par is not None:
                par.children[key] = node
            nodes.append(node)
        return nodes[0]

    def _insert_observation_nodes(self, tree, root):
        """Closed loop: every visited action node gets its single observation child (key str(observation), prior 0,
        the action node's own statistics -- both are updated by exactly the same episodes) holding the action node's
        children (mcts.py:267-273)."""
        from rl_agents_amd.agents.tree_search.abstract import Node
        env0 = getattr(self, "_last_env", None)
        if env0 is None:
            raise RuntimeError("closed-loop tree export needs the environment of the last plan")
        stack = [(tree, copy.deepcopy(getattr(env0, "unwrapped", env0)))]
        while stack:
            node, env = stack.pop()
            for action, child in list(node.children.items()):
                if child.count <= 0:
                    continue
                e = copy.deepcopy(env)
                observation = e.step(action)[0]
                obs_node = Node(child, str(observation), child.count, child.value, child.depth)
                obs_node.prior = 0
                obs_node.children, child.children = child.children, {str(observation): obs_node}
                for grandchild in obs_node.children.values():
                    grandchild.parent = obs_node
                stack.append((obs_node, e))

    def _export_open_loop(self, root=0):
        self.require_device_tree()
        arrays = self.relabel_tree(self.models.ctx.uct_tree(root), getattr(self, "_last_model", None))
        if self._last_tables is None:
            # finite-MDP models: every node also learns the state its action sequence reaches (Node.get_obs_visits)
            transition, roots = None, getattr(self, "_last_roots", None)
            if roots is not None and not device_model.is_cartpole(self._last_env):
                transition = np.asarray(device_model.finite_mdp_of(self._last_env).transition)
            return build_tree(arrays, "value", prior=policy_probabilities(self.prior_policy, self._last_actions), planner=self,
                              transition=transition, root_state=None if transition is None else int(roots[root]))
        # per-state priors: a child's prior is the prior agent's probability of its action in the state of its
        # parent (mcts.py:237-246); states follow from the root state and the deterministic transitions
        transition, prior, roots = self._last_tables
        tree = build_tree(arrays, "value", planner=self)
        tree.prior, tree.state = 1.0, int(roots[root])
        stack = [tree]
        while stack:
            node = stack.pop()
            for action, child in node.children.items():
                child.state = int(transition[node.state, action])
                child.prior = float(prior[node.state, action])
                stack.append(child)
        return tree


class MCTSAgent(AbstractTreeSearchAgent):
    """Drop-in for ``rl_agents.agents.tree_search.mcts.MCTSAgent``."""

    def make_planner(self):
        for key in ("prior_policy", "rollout_policy"):
            policy_probabilities(self.config[key], 2)           # validates the policy type early
        return MCTS(self.env, self.config["prior_policy"], self.config["rollout_policy"], self.config)

    @classmethod
    def default_config(cls):
        config = super(MCTSAgent, cls).default_config()
        config.update({"budget": 100, "horizon": None, "prior_policy": {"type": "random_available"},
                       "rollout_policy": {"type": "random_available"}, "env_preprocessors": []})
        return config
