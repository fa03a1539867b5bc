"""Batched evaluation of N environments THAT EACH OWN THEIR FINITE MDP -- and change it at every step.

The north-star environment is "highway-v0 as a finite MDP": ``to_finite_mdp()`` rebuilds the environment's own
time-to-collision table from the current traffic at EVERY step, and every agent of the reference re-reads it there
(``ValueIterationAgent.act`` re-converts and re-solves, dynamic_programming/value_iteration.py:29-35; the tree-search agents
step deep copies of the live env, tree_search/abstract.py:59-62).  The reference evaluates one such environment per process
(``Evaluation.run_episodes``, trainer/evaluation.py:139-194; ``scripts/experiments.py:102-106`` fans processes out).

Here N environments advance in lock-step and share ONE launch per step:

    per step, for the live episodes:   mdp_i = env_i.to_finite_mdp()                 (host: the reference's own extraction)
                                       batch model <- the tables that changed        (mp_model_update_tables: the delta of
                                                                                      a batch is each episode's own table)
                                       ONE batched plan, one MDP per root            (mp_vi_solve_batch + argmax /
                                                                                      mp_uct_plan_models / mp_opd_plan_models /
                                                                                      mp_olop_plan_models / mp_brue_plan_models /
                                                                                      mp_ropd_plan_models; on request
                                                                                      mp_gape_plan_models / mp_ss_plan_models /
                                                                                      mp_gape_plan_stochastic_models)
                                       env_i.step(action_i)                          (host: the environments are host objects)

Episode i draws from the generator a sequential ``Evaluation`` would give agent i (``np_random(sim_seed + i)``,
evaluation.py:375), continued from step to step, so the batch reproduces N sequential (environment, agent) loops action for
action (tests/test_gpu_per_episode_eval.py) -- and the unmodified reference's, on tests/golden/per_episode.npz.

Supported agents of this package: ``ValueIterationAgent``, ``MCTSAgent`` (``step_strategy`` "reset" or "subtree": the kept
subtrees of the live episodes are carried from plan to plan by ``mp_uct_step_tree_select``, with the counts, values, children and
stored priors they had, as abstract.py:172-206 keeps them whatever the table has become; ``closed_loop`` with "reset" plans open
loop and takes the first action -- the closed-loop plan's on a deterministic model),
``MCTSWithPriorPolicyAgent`` (round 6: the prior agent -- value iteration in the reference's own vi_prior.json -- is re-solved
for EVERY episode's table at every step, as mcts_with_prior.py:47-54 does through ``prior_agent.act``: ``mp_vi_solve_batch``,
the Boltzmann rows with numpy on the host -- the reference's distribution is numpy's ``exp``, whose SIMD implementation no
device restatement can be checked against -- and ``mp_policy_load`` over the batch model's global states),
``DeterministicPlannerAgent``, ``OLOPAgent`` (OLOP / KL-OLOP: the planner's own thresholds and initial bounds, its
continuation and its exceptions, as ``OLOP.plan_batch``) and ``BRUEAgent`` (which draws over ALL actions, brue.py:27: its
batch model carries neither the availability table nor the listing order, as ``BRUE.model_for`` loads it) and
``DiscreteRobustPlannerAgent`` (which builds its M candidate models again before every plan, robust.py:68-71: every episode owns a
SET of M tables per step, held as one joint batch model -- ``mp_model_load_joint_batch`` / ``mp_model_update_joint_tables`` --
and planned on by ``mp_ropd_plan_models``; see :meth:`PerEpisodeEvaluation._sync_joint`); on request, by name --
``PerEpisodeEvaluation(..., kind="gape")`` / ``kind="ss"`` -- ``MDPGapEAgent`` (``mp_gape_plan_models``) and ``SparseSamplingAgent``
(``mp_ss_plan_models``): the loop has always refused the two and still does unasked, since earlier code may rely on the refusal;
``kind="gape_stoch"`` -- ``PerEpisodeStochasticMDPGapEAgent`` (MDP-GapE with ``max_next_states_count`` 1..32,
``mp_gape_plan_stochastic_models``; ``StochasticMDPGapEAgent`` itself stays refused under any kind);
their batch model carries the availability table in listing order, as OLOP's, and the one call per lock-step is the planner's own
``plan_on`` with its exceptions; environments: deterministic finite MDPs of one (S, A) shape, with or without restricted /
re-ordered action sets (``get_available_actions``: the restriction must be the same table for every episode, as it is for
grids of one shape -- device_model.availability_of).
"""
import time

import numpy as np

from rl_agents_amd import device_model, native


def restrict_and_renormalise(tables, available):
    """``agent_policy_available`` (mcts_with_prior.py:56-62) for every row of ``tables`` [..., S, A] at once: the probabilities
    of the listed actions (``available`` bool [S, A], columns in listing order) divided by ``np.sum`` of them, zeros elsewhere.
    numpy sums fewer than 8 numbers one after the other from 0.0, and adding the +0.0 that stands in for an unlisted action
    changes nothing, so the sequential sum over ALL columns of the masked row is the reference's sum over the listed ones;
    exactly 8 listed actions (|A| = 8, everything available) take numpy's 8-accumulator form ((0+1)+(2+3))+((4+5)+(6+7))."""
    available = np.asarray(available).astype(bool)
    masked = np.where(available, tables, 0.0)
    a = masked.shape[-1]
    if a > 8:
        raise NotImplementedError("restrict_and_renormalise: |A| = {} > 8".format(a))
    den = masked[..., 0]
    for k in range(1, a):
        den = den + masked[..., k]
    if a == 8:
        m = [masked[..., k] for k in range(8)]
        pair = ((m[0] + m[1]) + (m[2] + m[3])) + ((m[4] + m[5]) + (m[6] + m[7]))
        den = np.where(available.all(axis=-1), pair, den)
    return masked / den[..., None]


def boltzmann_prior_rows(q, order, temperature, available):
    """The rows the loop uploads for a ``ValueIterationAgent`` prior: ``q`` [..., S, A] in DEVICE columns (column j = action
    ``order[j]``; ``order`` None: ascending) -> softmax(Q / temperature) [..., S, A] in device columns, restricted to
    ``available`` (bool [S, A], device columns, or None) and renormalised.  The sequential agent computes ``exp`` and the row
    sum over the actions in ACTION-ID order (``ValueIterationAgent.policy_table``) and permutes afterwards
    (``MCTSWithPriorPolicyAgent.policy_tables``): a sum over permuted columns differs in the last bits for any order but a swap
    of the first two, so ``q`` goes back to action-id order first -- as a contiguous array, since numpy's ``exp`` and its
    8-accumulator row sum are what they are on contiguous rows only."""
    q = np.asarray(q, dtype=np.float64)
    if order is not None:
        order = np.asarray(order, dtype=np.int64)
        inverse = np.empty_like(order)
        inverse[order] = np.arange(len(order))
        q = np.ascontiguousarray(q[..., inverse])
    z = np.exp((q - q.max(axis=-1, keepdims=True)) / temperature)
    tables = z / z.sum(axis=-1, keepdims=True)
    if order is not None:
        tables = tables[..., order]
    if available is not None:
        tables = restrict_and_renormalise(tables, available)
    return tables


class PerEpisodeEvaluation(object):
    def __init__(self, envs, agent, sim_seed=0, max_steps=None, kind=None):
        """``envs``: N environments exposing a deterministic finite MDP (``.mdp`` or ``to_finite_mdp()``) of one shape;
        ``agent``: an agent of this package built on ``envs[0]`` -- the template: its class and configuration are what every
        episode's agent would be.  ``sim_seed``: episode i's agent is seeded ``sim_seed + i`` -- or ``sim_seed[i]``, given one seed
        per episode.  ``max_steps``: episode length cap (default: the env's ``max_steps``, else 100).  ``kind``: what the loop does
        with the planner, by name -- the planner class's ``per_episode_kind`` (the default, None: that kind, or the refusal of
        a planner that declares none) or its ``per_episode_kind_on_request`` ("gape" for ``MDPGapEAgent``, "ss" for
        ``SparseSamplingAgent``, "gape_stoch" for ``PerEpisodeStochasticMDPGapEAgent``: planners this loop refuses unasked)."""
        self.envs, self.agent = list(envs), agent
        if not self.envs:
            raise ValueError("at least one environment")
        self.n = len(self.envs)
        self.sim_seed = sim_seed
        if np.ndim(sim_seed) != 0 and len(sim_seed) != self.n:
            raise ValueError("sim_seed: one seed, or one per episode ({} for {} episodes)".format(len(sim_seed), self.n))
        self.max_steps = int(max_steps or device_model.env_max_steps(self.envs[0]) or 100)
        self.vi = not hasattr(agent, "planner")
        planner = None if self.vi else agent.planner
        if not getattr(planner, "supports_per_episode_tables", True):
            raise NotImplementedError("per-episode tables: {} keeps its planner state (graph, bounds, state values) from plan to "
                                      "plan, and a kept state was built on the previous step's table".format(type(planner).__name__))
        # every planner class says what this loop does with it (AbstractPlanner.per_episode_kind)
        self.subtree = False
        self.kind = "vi" if self.vi else planner.per_episode_kind
        if kind is not None:
            offered = ["vi"] if self.vi else [k for k in (planner.per_episode_kind, getattr(planner, "per_episode_kind_on_request", None))
                                              if k is not None]
            if kind not in offered:
                raise ValueError("per-episode tables: kind {!r} is not one {} offers ({})".format(
                    kind, "value iteration" if self.vi else type(planner).__name__, ", ".join(repr(k) for k in offered) or "none"))
            self.kind = kind
        if self.kind is None:
            raise NotImplementedError("per-episode tables: this loop has no kind that plans {} on one model per episode, "
                                      "and would run the optimistic planner in its place".format(type(planner).__name__))
        if not self.vi:
            cfg = planner.config
            # MCTS keeps its subtrees as the reference does (abstract.py:172-206: count, value, children and stored priors of the
            # kept nodes, whatever the table has become); closed loop WITH kept subtrees is broken in the reference itself, and the
            # other planners' kept trees hold bounds computed on the previous table
            self.subtree = cfg.get("step_strategy", "reset") == "subtree" and self.kind == "uct" and not cfg.get("closed_loop")
            if cfg.get("step_strategy", "reset") != "reset" and not self.subtree:
                raise NotImplementedError("per-episode tables: the tree of the previous step was built on the previous table; "
                                          "step_strategy must be 'reset'")
            # (closed_loop with "reset" plans open loop and takes the first action: on a deterministic model that is the closed-loop
            # plan's first action, MCTS.supports_device_loop)
        # MCTSWithPriorPolicyAgent: the planner's policies are the prior agent's per-state distribution (mcts_with_prior.py:31-32)
        self.with_prior = self.kind == "uct" and getattr(planner, "policy_source", None) is not None
        self.ctx = (device_model.ModelCache().ctx if self.vi else planner.models.ctx)
        self.model = None
        self.uploads = 0            # MDP tables sent to the device (initial load + per-step deltas)
        self._tables = None
        # where a run's wall time goes: the environments' own extraction (host), comparing + sending tables, the batched plan
        # (launches + results), stepping the environments (host)
        self.seconds = dict(extract=0.0, upload=0.0, plan=0.0, env_step=0.0)

    # ------------------------------------------------------------------------------------------------ model extraction
    def _extract(self, i):
        """(spec or None, state, steps) of environment i as it is now.  spec -- transition [S,A] in device column order, reward,
        terminal, availability, listing order -- is None when the environment's MDP vouches, through ``tables_version``
        (envs/finite_mdp.py), that its tables are the ones this batch already holds for episode i: nothing is re-built, compared
        or sent for it (the whole-table comparison per episode per step was the step time of a static batch)."""
        env = self.envs[i]
        mdp = device_model.finite_mdp_of(env)
        if mdp.mode != "deterministic":
            raise TypeError("per-episode evaluation plans on deterministic finite MDPs, got mode '{}'".format(mdp.mode))
        state, steps = int(mdp.state), int(getattr(getattr(env, "unwrapped", env), "steps", 0) or 0)
        version = getattr(mdp, "tables_version", None)
        if version is not None and (not isinstance(version, tuple) or version[0] is None):
            version = None
        # (availability_of cross-checks the env's listing; BRUE never asks the environment: brue.py:27 draws over action_space.n)
        available, order = (None, None) if self.vi or self.kind == "brue" else device_model.availability_of(env, mdp)
        if self.model is not None and version is not None and self._versions[i] == version:
            return None, state, steps
        if self.kind == "uct":
            self.agent.planner._env_order = order           # (what MCTS.model_for notes for restricted_policy_tables)
            if order is not None and not self.with_prior and self.agent.planner.prior_policy["type"] == "random":
                order = None                                # policy type `random` lists np.arange(n) (mcts.py:46-57)
        spec = device_model.spec_from_mdp(mdp, max_steps=device_model.env_max_steps(env), available=available, action_order=order)
        spec.version = version
        return spec, state, steps

    def _extract_joint(self, i):
        """(set or None, joint state [M]) of environment i as it is now: its M candidate models, built the way the agent builds
        them before every plan (``preprocess_env(true_env, preprocessors)`` for each entry of ``config["models"]``,
        robust.py:68-71).  set -- dict(t [M,S,A], r, term [M,S], masks, rule, max_steps, version) -- is None when every model's
        MDP vouches through ``tables_version`` that its tables are the ones the batch holds for episode i."""
        from rl_agents_amd.agents.common.factory import preprocess_env
        env = self.envs[i]
        models = [preprocess_env(env, preprocessors) for preprocessors in self.agent.config["models"]]
        if not models:
            raise TypeError("the discrete robust planner plans on a JointEnv of at least one model")
        mdps = [device_model.finite_mdp_of(e) for e in models]
        for mdp in mdps:
            if mdp.mode != "deterministic":
                raise TypeError("every model must be a deterministic finite MDP, got mode '{}'".format(mdp.mode))
        state = [int(mdp.state) for mdp in mdps]
        versions = []
        for mdp in mdps:
            v = getattr(mdp, "tables_version", None)
            versions.append(v if isinstance(v, tuple) and v[0] is not None else None)
        version = None if any(v is None for v in versions) else tuple(versions)
        # JointEnv.get_available_actions (robust.py:22-25) lists list(set().union(...)) of what each model lists in its own state:
        # the models' own listing orders are lost in the set, and the device expands the union in ascending order
        avail = [device_model.availability_of(e, mdp) for e, mdp in zip(models, mdps)]
        masks = [a[0] for a in avail]
        rows = []
        for (mask, order), mdp in zip(avail, mdps):
            n_actions = np.asarray(mdp.reward).shape[-1]
            seq = range(n_actions) if order is None else order
            rows.append([int(a) for a in seq if mask is None or mask[int(mdp.state), int(a)]])
        listed = list(set().union(*rows))
        if listed != sorted(listed):
            raise NotImplementedError("per-episode tables: the discrete robust planner plans on a joint environment that lists its "
                                      "actions in ascending order, got {}".format(listed))
        if self.model is not None and version is not None and self._versions[i] == version:
            return None, state
        shapes = {np.asarray(m.transition).shape for m in mdps}
        if len(shapes) != 1:
            raise ValueError("all models must share the state and action spaces, got tables of shapes {}".format(shapes))
        rules = {getattr(m, "done_rule", "source") for m in mdps}
        if len(rules) != 1:
            raise ValueError("all models of a joint environment must share one done_rule, got {}".format(sorted(rules)))
        limits = {device_model.env_max_steps(e) for e in models}
        if len(limits) != 1:
            raise ValueError("all models of a joint environment must share one max_steps, got {}".format(sorted(limits)))
        return dict(t=np.stack([np.asarray(m.transition, dtype=np.int64) for m in mdps]),
                    r=np.stack([np.asarray(m.reward, dtype=np.float64) for m in mdps]),
                    term=np.stack([np.asarray(m.terminal).reshape(-1).astype(np.uint8) for m in mdps]),
                    masks=masks, rule=rules.pop(), max_steps=limits.pop(), version=version), state

    def _check_joint(self, sp, first):
        if sp["t"].shape != first["t"].shape:
            raise ValueError("every environment of the batch must have the same number of models, states and actions")
        same_avail = all((a is None) == (b is None) and (a is None or (a.shape == b.shape and
                                                                       np.asarray(a).tobytes() == np.asarray(b).tobytes()))
                         for a, b in zip(sp["masks"], first["masks"]))
        if not (same_avail and sp["rule"] == first["rule"] and sp["max_steps"] == first["max_steps"]):
            raise NotImplementedError("per-episode evaluation: the episodes' environments must restrict the actions of each model "
                                      "identically and share done_rule / max_steps")

    def _sync_joint(self, live):
        """The robust planner's :meth:`_sync_model`: the joint batch model holds one SET of M tables per episode; returns
        (joint states [N, M], steps).  One upload is one episode's set."""
        n = self.n
        m = len(self.agent.config["models"])
        states, steps = np.zeros((n, max(m, 1)), np.int32), np.zeros(n, np.int32)
        sets = [None] * n
        c0 = time.perf_counter()
        for i in live:
            sets[i], states[i] = self._extract_joint(i)
        self.seconds["extract"] += time.perf_counter() - c0
        if self.model is None:
            first = self._first_spec = sets[live[0]]
            self._tables = dict(t=np.zeros((n,) + first["t"].shape, np.int64), r=np.zeros((n,) + first["r"].shape, np.float64),
                                term=np.zeros((n,) + first["term"].shape, np.uint8))
            self._versions = [None] * n
            for i in live:
                self._check_joint(sets[i], first)
                self._tables["t"][i], self._tables["r"][i], self._tables["term"][i] = sets[i]["t"], sets[i]["r"], sets[i]["term"]
                self._versions[i] = sets[i]["version"]
            available = None
            if any(a is not None for a in first["masks"]):      # (a model whose env has no get_available_actions lists everything)
                per_set = np.stack([np.ones(first["t"].shape[1:], dtype=bool) if a is None else np.asarray(a).astype(bool)
                                    for a in first["masks"]])
                available = np.broadcast_to(per_set, (n,) + per_set.shape)
            self.model = self.ctx.load_joint_batch(self._tables["t"], self._tables["r"], self._tables["term"],
                                                   done_rule=first["rule"], available=available)
            self.uploads += len(live)
            return states, steps
        changed = []
        tb = self._tables
        for i in live:
            sp = sets[i]
            if sp is None:
                continue
            self._check_joint(sp, self._first_spec)
            self._versions[i] = sp["version"]
            # (as in _sync_model: the CONTENT decides what is sent)
            if not (tb["t"][i].tobytes() == sp["t"].tobytes() and tb["r"][i].tobytes() == sp["r"].tobytes()
                    and tb["term"][i].tobytes() == sp["term"].tobytes()):
                tb["t"][i], tb["r"][i], tb["term"][i] = sp["t"], sp["r"], sp["term"]
                changed.append(i)
        self._send_changed(changed)
        return states, steps

    def _send_changed(self, changed):
        """Contiguous runs of changed episodes: one mp_model_update_tables (mp_model_update_joint_tables) each."""
        tb = self._tables
        k = 0
        while k < len(changed):
            j = k
            while j + 1 < len(changed) and changed[j + 1] == changed[j] + 1:
                j += 1
            lo, hi = changed[k], changed[j] + 1
            self.model.update_tables(lo, tb["t"][lo:hi], tb["r"][lo:hi], tb["term"][lo:hi])
            k = j + 1
        self.uploads += len(changed)

    def _sync_model(self, live):
        """Bring the batch model up to date with the live episodes' environments; returns (states, steps)."""
        if self.kind == "ropd":
            return self._sync_joint(live)
        n = self.n
        states, steps = np.zeros(n, np.int32), np.zeros(n, np.int32)
        specs = [None] * n
        c0 = time.perf_counter()
        for i in live:
            specs[i], states[i], steps[i] = self._extract(i)
        self.seconds["extract"] += time.perf_counter() - c0
        if self.model is None:
            # every slot needs a table: finished episodes cannot be among them at the first step
            first_spec = self._first_spec = specs[live[0]]
            s, a = first_spec.n_states, first_spec.n_actions
            self._tables = dict(t=np.zeros((n, s, a), np.int64), r=np.zeros((n, s, a), np.float64), term=np.zeros((n, s), np.uint8))
            self._versions = [None] * n
            for i in live:
                self._check_shape(specs[i], first_spec)
                self._tables["t"][i], self._tables["r"][i], self._tables["term"][i] = specs[i].transition, specs[i].reward, specs[i].terminal
                self._versions[i] = specs[i].version
            self.model = self.ctx.load_table_batch(self._tables["t"], self._tables["r"], self._tables["term"],
                                                   done_rule=first_spec.done_rule, max_steps=first_spec.max_steps)
            self.model.action_order = first_spec.action_order
            self._available = None if first_spec.available is None else first_spec.available.astype(bool)
            if self._available is not None and self.kind in ("opd", "olop", "gape", "ss", "gape_stoch"):
                # (MCTS reads availability through its policies, mcts.py:59-97: see _uct_policy)
                self.model.set_available(np.tile(self._available, (n, 1)))
            self.uploads += len(live)
            return states, steps
        changed = []
        tb = self._tables
        for i in live:
            sp = specs[i]
            if sp is None:                                   # same tables_version as what the batch holds: nothing to do
                continue
            self._check_shape(sp, self._first_spec)
            self._versions[i] = sp.version
            # (a new version is not yet a new table -- an environment may assign the same arrays again -- so the CONTENT decides
            # what is sent; what the version spares is this comparison for tables that did not change.  Compared as bytes: three
            # np.array_equal calls on 600-element tables were 10 us per episode, a third of a lock-step's "upload")
            tb_t, tb_r, tb_m = tb["t"][i], tb["r"][i], tb["term"][i]
            if not (tb_t.tobytes() == sp.transition.tobytes() and tb_r.tobytes() == sp.reward.tobytes()
                    and tb_m.tobytes() == sp.terminal.tobytes()):
                tb_t[...], tb_r[...], tb_m[...] = sp.transition, sp.reward, sp.terminal
                changed.append(i)
        self._send_changed(changed)
        if changed and getattr(self, "_policy", None) is not None:      # fused policy records hold the old transitions
            self._policy.close()
            self._policy = None
        return states, steps

    def _check_shape(self, spec, first):
        if spec.reward.shape != first.reward.shape:
            raise ValueError("every environment of the batch must have the same number of states and actions")
        # (bytes, not np.array_equal: this runs per episode per step)
        same_order = (spec.action_order is None) == (first.action_order is None) and \
            (spec.action_order is None or spec.action_order.tobytes() == first.action_order.tobytes())
        same_avail = (spec.available is None) == (first.available is None) and \
            (spec.available is None or (spec.available.shape == first.available.shape and spec.available.tobytes() == first.available.tobytes()))
        if not (same_order and same_avail and spec.done_rule == first.done_rule and spec.max_steps == first.max_steps):
            raise NotImplementedError("per-episode evaluation: the episodes' environments must list / restrict their actions "
                                      "identically and share done_rule / max_steps")

    # ------------------------------------------------------------------------------------------------ one batched plan
    def _uct_policy(self):
        """Per-state policy tables over the GLOBAL states for environments that restrict their actions (the same [S, A]
        rows for every episode), re-fused whenever a table changed."""
        planner = self.agent.planner
        if getattr(self, "_policy", None) is None:
            self.model.available = self._available
            prior, rollout, listed, slots = planner.restricted_policy_tables(self.model, self._available)
            # [S_each, A] rows over LOCAL states: the same for every episode (mp_policy_load_rows tiles them on the device)
            self._policy = self.ctx.load_policy(self.model, prior, rollout, listed=listed, rollout_slots=slots)
        return self._policy

    def _prior_tables(self, live):
        """[N, S, A] (device column order): the prior agent's action distribution in every state of every live episode's OWN
        table -- what ``agent_policy_available`` (mcts_with_prior.py:47-62) returns when asked about a copy of that episode's
        environment: ``prior_agent.env = state; prior_agent.act(obs); prior_agent.action_distribution(obs)``, restricted to the
        listed actions and renormalised where the environment restricts them."""
        from rl_agents_amd.agents.dynamic_programming.value_iteration import ValueIterationAgent
        from rl_agents_amd.agents.tree_search.mcts_with_prior import tabulate_prior_agent
        model, pa = self.model, self.agent.prior_agent
        n, s, a = self.n, model.S_each, model.A
        if type(pa) is ValueIterationAgent:
            # its act() re-converts and re-solves (value_iteration.py:29-35) and its distribution is Boltzmann over that Q table
            # (ValueIterationAgent.policy_table): N solves in one launch, the softmax rows in one numpy expression -- numpy's own
            # exp and its own summation order over the |A| entries of a row IN ACTION-ID ORDER, exactly as the single agent
            # computes them (boltzmann_prior_rows)
            q, _ = self.ctx.vi_solve_batch(model, pa.config["gamma"], pa.config["iterations"])
            return boltzmann_prior_rows(q, getattr(model, "action_order", None), pa.config.get("temperature", 1.0), self._available)
        else:
            if getattr(self, "_prior_cache", None) is None:
                self._prior_cache = np.zeros((n, s, a))
            tables = self._prior_cache
            order = getattr(model, "action_order", None)
            for i in live:
                pa.env = self.envs[i]                    # "reset prior agent environment" (:49)
                t = tabulate_prior_agent(pa, s, a)
                tables[i] = t if order is None else t[:, order]
        if self._available is not None:
            tables = restrict_and_renormalise(tables, self._available)
        return tables

    def _step_kept_trees(self, live):
        """step_strategy "subtree" for a batch whose episodes end at different steps: the live episodes' trees of the previous
        plan, each stepped by the action its episode executed (abstract.py:172-206), become the roots of this plan, in its order
        (mp_uct_step_tree_select).  The first step plans fresh trees.  The trees live in the context's workspaces, which every
        planner of the process shares: the planner claims them after each plan, and a plan of another one between two steps is
        an error here rather than a tree silently started afresh."""
        planner = self.agent.planner
        planner.about_to_plan()
        if self._kept_live is None:
            self.ctx.uct_reset_tree()
            return
        if not planner.owns_device_tree():
            raise RuntimeError("per-episode tables, step_strategy 'subtree': another planner of the process has planned on this "
                               "context since the previous step, and the kept trees are gone")
        position = {episode: j for j, episode in enumerate(self._kept_live)}
        source = np.asarray([position[i] for i in live], dtype=np.int32)
        # (the executed action as the device labels it: the batch model's column order, planner.device_actions -- the plans'
        # first entries before they were translated for the environment)
        self.ctx.uct_step_tree_select(source, self._kept_labels[source])

    def _plan(self, live, states, steps):
        """First actions (environment action ids) of the live episodes + planner env steps of this plan."""
        from rl_agents_amd.agents.tree_search.mcts import policy_probabilities
        agent, model = self.agent, self.model
        idx = np.asarray(live, dtype=np.int32)
        if self.vi:
            q, _ = self.ctx.vi_solve_batch(model, agent.config["gamma"], agent.config["iterations"])
            return np.array([int(np.argmax(q[i, states[i]])) for i in live], dtype=np.int64), 0   # value_iteration.py:35
        planner = agent.planner
        cfg = planner.config
        rng = np.ascontiguousarray(self.rng[idx])
        if self.subtree:
            self._step_kept_trees(live)

        def plan_with(policy):
            # per-state policies.  With kept subtrees every plan, the first included, takes the kernel that STORES a node's priors
            # and child set at expansion (mp_uct_plan_stochastic_policy; it takes deterministic tables): mp_uct_plan_policy looks
            # both up by the state the descent is in, which is only right while table and policy stay what they were
            roots = idx * model.S_each + states[idx]
            if self.subtree:
                return self.ctx.uct_plan_stochastic(model, roots, cfg["episodes"], cfg["horizon"], cfg["gamma"], cfg["temperature"],
                                                    None, None, rng, closed_loop=False, root_steps=steps[idx], max_plan_len=1,
                                                    policy=policy)
            return self.ctx.uct_plan(model, roots, cfg["episodes"], cfg["horizon"], cfg["gamma"], cfg["temperature"], None, None, rng,
                                     root_steps=steps[idx], max_plan_len=1, policy=policy)
        if self.with_prior:
            tables = np.ascontiguousarray(self._prior_tables(live).reshape(self.n * model.S_each, model.A))
            listed = None if self._available is None else np.tile(self._available, (self.n, 1))
            model.available = self._available
            policy = self.ctx.load_policy(model, tables, tables, listed=listed)
            try:
                out = plan_with(policy)
            finally:
                policy.close()
        elif self.kind == "uct":
            if self._available is not None:
                out = plan_with(self._uct_policy())
            else:
                pp, rp = policy_probabilities(planner.prior_policy, model.A), policy_probabilities(planner.rollout_policy, model.A)
                out = self.ctx.uct_plan(model, states[idx], cfg["episodes"], cfg["horizon"], cfg["gamma"], cfg["temperature"], pp, rp,
                                        rng, root_steps=steps[idx], max_plan_len=1, model_index=idx)
        else:
            # the planner's own call: root i plans on MDP i (the robust planner: on set i, from the joint state of its M models;
            # its plans are the env's action ids -- the joint env lists ascending) and its exceptions are the planner's
            out = planner.plan_on(model, states[idx], steps[idx], rng, model_index=idx, max_plan_len=1)
            if planner.draws_survive_errors:            # (the draws made before a failing step are made: OLOP.plan_batch)
                self.rng[idx] = rng
            planner.raise_for_result(out)
        self.rng[idx] = rng
        if (out["plan_len"] < 1).any():
            raise Exception("The agent did not plan any action")             # evaluation.py:168-170
        first = out["plans"][:, 0].astype(np.int64)
        if self.subtree:
            planner.claim_device_tree()
            self._kept_live, self._kept_labels = list(live), out["plans"][:, 0].astype(np.int32)
        order = getattr(model, "action_order", None)
        if order is not None:
            first = np.asarray(order, dtype=np.int64)[first]
        return first, int(out["env_steps"].sum())

    # ------------------------------------------------------------------------------------------------ the loop
    def run(self):
        """Run every episode to termination / truncation (each environment is reset first).  Returns dict(returns,
        discounted_returns, lengths, actions [N, max_steps] (-1 padded), wall / extract / update / plan seconds,
        planner_env_steps, uploads)."""
        n, T = self.n, self.max_steps
        for env in self.envs:
            env.reset()
        if np.ndim(self.sim_seed) == 0:
            self.rng = native.seed_sequence_states((), self.sim_seed, n)    # np_random(sim_seed + i), evaluation.py:375
        else:                                                               # one seed per episode
            self.rng = np.concatenate([native.seed_sequence_states((), int(seed), 1) for seed in self.sim_seed])
        self._kept_live = self._kept_labels = None                          # (subtree: the episodes and first actions of the last plan)
        alive = np.ones(n, dtype=bool)
        returns, disc, lengths = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
        actions = np.full((n, T), -1, dtype=np.int32)
        gamma = float(self.agent.config.get("gamma", 1))
        t_extract = t_plan = 0.0
        planner_steps = 0
        t0 = time.perf_counter()
        for t in range(T):
            live = [int(i) for i in np.flatnonzero(alive)]
            if not live:
                break
            c0 = time.perf_counter()
            before = self.seconds["extract"]
            states, steps = self._sync_model(live)
            c1 = time.perf_counter()
            self.seconds["upload"] += (c1 - c0) - (self.seconds["extract"] - before)
            acts, es = self._plan(live, states, steps)
            self.ctx.synchronize()
            c2 = time.perf_counter()
            self.seconds["plan"] += c2 - c1
            t_extract += c1 - c0
            t_plan += c2 - c1
            planner_steps += es
            c3 = time.perf_counter()
            for i, a in zip(live, acts):
                _, reward, terminated, truncated, _ = self.envs[i].step(int(a))
                returns[i] += reward
                disc[i] += reward * gamma ** t
                actions[i, t] = int(a)
                lengths[i] += 1
                if terminated or truncated or lengths[i] >= T:
                    alive[i] = False
            self.seconds["env_step"] += time.perf_counter() - c3
        wall = time.perf_counter() - t0
        if not self.vi:
            self.agent.planner.env_steps += planner_steps
        return dict(returns=returns, discounted_returns=disc, lengths=lengths, actions=actions, wall_seconds=wall,
                    extract_update_seconds=t_extract, plan_seconds=t_plan, planner_env_steps=planner_steps, uploads=self.uploads,
                    seconds=dict(self.seconds),
                    fps=float(lengths.sum()) / wall if wall > 0 else 0.0)

    def close(self):
        if getattr(self, "_policy", None) is not None:
            self._policy.close()
            self._policy = None
        if self.model is not None:
            self.model.close()
            self.model = None
