"""Every call the planners and the per-episode loop make into the binding, pinned against a recorded run (host only, no GPU,
no library), one layer above tests/test_binding_calls_host.py.

A recording stand-in takes the place of ``planner.models`` (a ``.ctx`` and a ``.get(spec)``) and of the ``Context`` methods the
planners call.  Each call is bound against the real method's signature and recorded in order -- method name, scalars, arrays
as dtype / shape / content -- and answered with a fixed pattern: plans of zeros, ``plan_len`` 1, ``env_steps`` = root index + 1,
every generator record advanced by 3.  A case may ask for a status code or negative BRUE plans on one root of one plan call.
The two graph-based planners construct ``native.GraphBasedPlanners`` / ``native.StochasticGraphBasedPlanners`` themselves, so
these classes have a recording stand-in of their own (GraphPlanners), whose calls are recorded with the context's.
What the planner returns, the generator records, ``planner.env_steps``, whether ``planner.last`` is the result, the tree claim,
the log lines and any exception are recorded with the calls.  The record of every case must equal tests/planner_calls.json, which
``python tests/test_planner_calls_host.py --write`` writes (the package first on PYTHONPATH is the one recorded).
"""
import copy
import functools
import hashlib
import inspect
import json
import logging
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # (after PYTHONPATH: it chooses the package)

from rl_agents_amd import native, runtime  # noqa: E402
from rl_agents_amd.agents.dynamic_programming.value_iteration import ValueIterationAgent  # noqa: E402
from rl_agents_amd.agents.robust.robust import DiscreteRobustPlannerAgent  # noqa: E402
from rl_agents_amd.agents.tree_search.brue import BRUEAgent  # noqa: E402
from rl_agents_amd.agents.tree_search.deterministic import DeterministicPlannerAgent  # noqa: E402
from rl_agents_amd.agents.tree_search.mcts import MCTSAgent  # noqa: E402
from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapEAgent, StochasticMDPGapEAgent  # noqa: E402
from rl_agents_amd.agents.tree_search.olop import OLOPAgent  # noqa: E402
from rl_agents_amd.agents.tree_search.state_aware import StateAwarePlannerAgent  # noqa: E402
from rl_agents_amd.envs.finite_mdp import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv  # noqa: E402
from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation  # noqa: E402
from tests import helpers  # noqa: E402

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "planner_calls.json")
A, S, WIDE = 3, 10, 9
RNG_STEP = 3
MODES = {"deterministic": native.MODE_DETERMINISTIC, "stochastic": native.MODE_STOCHASTIC, "sparse": native.MODE_SPARSE}
PLANS = {"uct_plan": "uct", "uct_plan_stochastic": "uct", "opd_plan": "opd", "ropd_plan": "opd", "olop_plan": "olop",
         "olop_plan_stochastic": "olop", "brue_plan": "brue", "gape_plan": "gape", "gape_plan_stochastic": "gape"}
OTHERS = ("uct_reset_tree", "uct_step_tree", "uct_step_tree_select", "load_policy", "load_joint", "load_table_batch",
          "load_joint_batch", "vi_solve_batch", "synchronize", "gape_tree", "gape_stoch_tree")


def _content(a):
    a = np.ascontiguousarray(a)
    if a.size <= 12:
        return a.reshape(-1).tolist()
    return "sha1:" + hashlib.sha1(a.tobytes()).hexdigest()[:16]


def describe(v):
    if isinstance(v, np.ndarray):
        return ["array", str(v.dtype), list(v.shape), _content(v)]
    if isinstance(v, (Model, Policy)):
        return [type(v).__name__.lower(), v.label]
    if isinstance(v, dict):
        return {str(k): describe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [describe(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return ["object", type(v).__name__]


class Model(object):
    """What the planners read of a native.Model; its own methods are recorded with the context's."""

    def __init__(self, ctx, mode, m, s, a, n_models=1, available=None):
        self.ctx, self.mode, self.M, self.S, self.A, self.B = ctx, mode, m, s * n_models, a, 0
        self.n_models, self.S_each = n_models, s
        self.label = "m{}".format(len(ctx.models))
        ctx.models.append(self)
        if available is not None:
            self.available = np.asarray(available).astype(bool)

    def _record(self, name, **named):
        self.ctx.calls.append([self.label + "." + name, describe(named)])

    def set_available(self, available):
        self._record("set_available", available=np.asarray(available))
        self.available = np.asarray(available).astype(bool)

    def set_episode_rules(self, done_rule="source", max_steps=0):
        self._record("set_episode_rules", done_rule=done_rule, max_steps=max_steps)

    def update_tables(self, first, transition, reward, terminal=None):
        self._record("update_tables", first=first, transition=transition, reward=reward, terminal=terminal)

    def close(self):
        pass


class Policy(object):
    def __init__(self, ctx):
        self.ctx, self.label = ctx, "p{}".format(ctx.policies)
        ctx.policies += 1

    def close(self):
        self.ctx.calls.append([self.label + ".close", {}])


class Ctx(object):
    """The recording stand-in of native.Context.  ``fail``: dict(call=k, root=i, status=code | negative=True) for the k-th
    plan call."""

    current = None          # what runtime.get_context() answers while a case runs (the VI loop asks it)

    def __init__(self, fail=None):
        self.calls, self.models, self.policies, self.plan_calls, self.fail = [], [], 0, 0, fail
        Ctx.current = self

    def __getattr__(self, name):
        if name not in PLANS and name not in OTHERS:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _call(self, name, *args, **kwargs):
        bound = inspect.signature(getattr(native.Context, name)).bind(self, *args, **kwargs)   # (TypeError as the binding's)
        bound.apply_defaults()                              # (an argument left out and its default handed over are one call)
        named = dict(bound.arguments)
        named.pop("self")
        self.calls.append([name, {k: describe(v) for k, v in named.items()}])
        if name in PLANS:
            return self._plan(name, **named)
        return getattr(self, "_" + name, lambda **kw: None)(**named)

    def _plan(self, name, model, root_state, rng_state, **kw):
        family = PLANS[name]
        n = np.asarray(root_state).shape[0]
        length = kw.get("max_plan_len")
        if length is None:
            length = max(int(kw["horizon"]), 1) * (2 if kw.get("closed_loop") else 1) if "horizon" in kw else 1
        if family == "gape":
            length = 1                                                  # (an MDP-GapE plan is one action)
        out = {}
        for key, dtype, tail, _ in native.RESULTS[family]:
            out[key] = np.zeros((n,) + tuple({"L": int(length), "A": model.A, "P": 2}[d] for d in tail), dtype)
        if "plan_len" in out:
            out["plan_len"][:] = 1
        out["env_steps"][:] = np.arange(n) + 1
        if "root_child_count" in out:
            out["root_child_count"][:] = np.arange(model.A) + 1         # (a relabelled result shows the permutation)
        if family == "gape":
            out["episodes_run"][:], out["best_challenger"][:], out["child_count"][:] = 3, (1, 2), np.arange(model.A) + 1
            out["child_lower"][:], out["child_upper"][:] = np.arange(model.A) / 10.0, np.arange(model.A) / 10.0 + 0.5
        fail = self.fail if self.fail and self.fail["call"] == self.plan_calls else None
        self.plan_calls += 1
        if fail and "status" in fail:
            out["status"][fail["root"]] = fail["status"]
        if fail and fail.get("negative"):
            out["plans"][fail["root"]] = -1
        assert isinstance(rng_state, np.ndarray) and rng_state.dtype == np.uint64 and rng_state.size == 6 * n
        rng_state += np.uint64(RNG_STEP)
        return out

    def _gape_tree(self, root, cap, keys=(-1, 0, 2, 5, 4), parent=(-1, 0, 0, 1, 2)):
        """A root with the arms 0 and 2 and a decision node under each."""
        n = len(keys)
        return dict(kind=np.asarray([0, 1, 1, 0, 0], np.uint8), parent=np.asarray(parent, np.int32), action=np.asarray(keys, np.int32),
                    depth=np.asarray([0, 0, 0, 1, 1], np.int32), count=np.arange(n, dtype=np.int64)[::-1] + 1,
                    cum=np.arange(n) / 4.0, mu_ucb=np.arange(n) / 8.0 + 0.5, mu_lcb=np.arange(n) / 8.0, vu=np.arange(n) + 0.5,
                    vl=np.arange(n) + 0.25, done=np.asarray([0, 0, 0, 0, 1], np.uint8), state=np.asarray([1, 1, 1, 5, 4], np.int32))

    def _gape_stoch_tree(self, root, cap):
        """A root with the arms 0 and 2; under arm 0 the placeholder left and the one observed state."""
        return self._gape_tree(root, cap, keys=(-1, 0, 2, -2, 4), parent=(-1, 0, 0, 1, 1))

    def _load_policy(self, model, prior, rollout, listed, rollout_slots):
        return Policy(self)

    def _load_joint(self, transitions, rewards, terminals, done_rule, available):
        m, s, a = np.asarray(transitions).shape
        return Model(self, native.MODE_DETERMINISTIC, m, s, a, available=available)

    def _load_table_batch(self, transition, reward, terminal, done_rule, max_steps):
        n, s, a = np.asarray(transition).shape
        return Model(self, native.MODE_DETERMINISTIC, 1, s, a, n_models=n)

    def _load_joint_batch(self, transitions, rewards, terminals, done_rule, available):
        n, m, s, a = np.asarray(transitions).shape
        return Model(self, native.MODE_DETERMINISTIC, m, s, a, n_models=n, available=available)

    def _vi_solve_batch(self, model, gamma, iterations, rtol, atol):
        i, s, a = np.meshgrid(np.arange(model.n_models), np.arange(model.S_each), np.arange(model.A), indexing="ij")
        return ((i * 7 + s * 3 + a * 5) % 11) / 10.0, np.full(model.n_models, 2, np.int32)


class GraphPlanners(object):
    """The recording stand-in of native.GraphBasedPlanners, which the graph-based planner constructs itself: ``create``, every
    ``plan``, ``info`` and ``close`` are bound against the real class and recorded with the context's calls.  A plan is answered
    as Ctx._plan answers one (``plans`` shows a relabelling); the context's ``fail`` may also name ``error`` (a NativeError's
    message) or ``set`` (result name -> the failing root's value)."""
    real, family, label = native.GraphBasedPlanners, "gbopd", "gbopd"

    def __init__(self, ctx, *args, **kwargs):
        self.ctx, self.max_count = ctx, 0
        named = self._record("create", self.real.__init__, (ctx,) + args, kwargs)
        self.model, self.n, self.K = named["model"], int(named["n_planners"]), int(named.get("max_next_states", 0))

    def _record(self, name, method, args, kwargs):
        bound = inspect.signature(method).bind(self, *args, **kwargs)       # (TypeError as the binding's)
        bound.apply_defaults()
        named = dict(bound.arguments)
        named.pop("self")
        named.pop("ctx", None)
        self.ctx.calls.append([self.label + "." + name, {k: describe(v) for k, v in named.items()}])
        return named

    def plan(self, *args, **kwargs):
        named = self._record("plan", self.real.plan, args, kwargs)
        ctx, n, rng = self.ctx, self.n, named["rng_state"]
        fail = ctx.fail if ctx.fail and ctx.fail["call"] == ctx.plan_calls else None
        ctx.plan_calls += 1
        if fail and "error" in fail:
            raise native.NativeError(native.MP_ERR_ARG, fail["error"])
        out = {}
        for key, dtype, tail, _ in native.RESULTS[self.family]:
            out[key] = np.zeros((n,) + tuple(int(named["sampling_timeout"]) for _ in tail), dtype)
        out["plans"][:] = (np.arange(out["plans"].size).reshape(out["plans"].shape) + 1) % self.model.A
        out["plan_len"][:] = 1
        out["env_steps"][:] = np.arange(n) + 1
        out["value_lower"][:], out["value_upper"][:] = np.arange(n) / 4.0, np.arange(n) / 4.0 + 0.5
        for key, value in (fail or {}).get("set", {}).items():
            out[key][fail["root"]] = value
        self.max_count += int(named.get("episodes", 0)) * int(named.get("horizon", 0))
        assert isinstance(rng, np.ndarray) and rng.dtype == np.uint64 and rng.size == 6 * n
        rng += np.uint64(RNG_STEP)
        return out

    def info(self):
        self.ctx.calls.append([self.label + ".info", {}])
        return dict(n_planners=self.n, n_states=self.model.S, n_actions=self.model.A, max_next_states=self.K, queue_cap=4,
                    n_edges=6, max_count=self.max_count)

    def close(self):
        self.ctx.calls.append([self.label + ".close", {}])


class StochasticGraphPlanners(GraphPlanners):
    real, family, label = native.StochasticGraphBasedPlanners, "gbop", "gbop"


class Models(object):
    """Stands where ``planner.models`` (device_model.ModelCache) is."""

    def __init__(self, ctx):
        self.ctx, self._held = ctx, {}

    def get(self, spec):
        key = spec.key()
        if key not in self._held:
            self.ctx.calls.append(["models.get", describe(dict(
                mode=spec.mode, transition=spec.transition, reward=spec.reward, terminal=spec.terminal, next=spec.next,
                done_rule=spec.done_rule, max_steps=spec.max_steps, available=spec.available, action_order=spec.action_order))])
            m = 1 if spec.transition.ndim == 2 or spec.mode != "deterministic" else spec.transition.shape[0]
            model = Model(self.ctx, MODES[spec.mode], m, spec.n_states, spec.n_actions,
                          available=spec.available if spec.mode == "deterministic" else None)
            model.action_order, model.spec = spec.action_order, spec
            self._held[key] = model
        return self._held[key]


class Log(logging.Handler):
    def __init__(self):
        super(Log, self).__init__(logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append([record.levelname, record.getMessage()])


# ---- environments and agents -----------------------------------------------------------------------------------------------------
def table(n_actions=A, shift=0, state=0):
    t, r, term = helpers.value_table(S, n_actions)
    return dict(mode="deterministic", transition=(t + shift) % S, reward=r, terminal=term, state=state)


def mask(n_actions=A):
    """Every state lists action 1; the others by a pattern that differs from state to state."""
    s, a = np.arange(S)[:, None], np.arange(n_actions)[None, :]
    return ((s + 2 * a) % 3 != 0) | (a == 1)


def plain_env(**kw):
    return FiniteMDPEnv(table(**kw))


def masked_env(n_actions=A, **kw):
    return MaskedFiniteMDPEnv(dict(table(n_actions, **kw), available=mask(n_actions)))


def stochastic_env(kind="stochastic", ordered=False):
    config = {k: v for k, v in helpers.stochastic_model(kind, S, A, False).items() if v is not None}
    env = OrderedMaskedFiniteMDPEnv(dict(config, available=mask(), listing_order=[2, 0, 1])) if ordered else FiniteMDPEnv(config)
    env.seed(3)
    return env


def ordered_env(**kw):
    return OrderedMaskedFiniteMDPEnv(dict(table(**kw), available=mask(), listing_order=[2, 0, 1]))


def rng_records(n):
    return (np.arange(n * 6, dtype=np.uint64).reshape(n, 6) + np.uint64(100)) * np.uint64(1000003)


def robust_config(**kw):
    other = table()["reward"][:, ::-1].copy()
    return dict(dict(budget=7, gamma=0.8, models=[[], [{"method": "copy_with_config", "args": {"reward": other}}]]), **kw)


UCT = dict(budget=8, episodes=4, horizon=2, gamma=0.8)
OLOP_KL = dict(budget=8, episodes=4, horizon=2, gamma=0.8, upper_bound=dict(type="kullback-leibler", time="global",
                                                                            threshold="2*np.log(time)"))
OLOP_HOEFFDING = dict(budget=8, episodes=4, horizon=2, gamma=0.8)
BRUE_CFG = dict(budget=6, horizon=2, gamma=0.8)
GAPE_CFG = dict(budget=8, episodes=4, horizon=2, gamma=0.8, accuracy=0.1)
GAPE_STOCH_CFG = dict(GAPE_CFG, max_next_states_count=2)


def gape_bound(**strings):
    return dict(upper_bound=dict(dict(type="kullback-leibler", time="global", threshold="2*np.log(time) + count",
                                      transition_threshold="0.1*np.log(time) + count"), **strings))


def with_stand_in(agent, ctx):
    agent.planner.models = Models(ctx)
    return agent.planner


# ---- one planner call and what it leaves -------------------------------------------------------------------------------------------
def plan_record(ctx, planner, call, rng):
    rec = {}
    out = None
    try:
        out = call()
        rec["result"] = describe(out)
    except Exception as e:     # noqa: BLE001 - type and message are the record
        rec["error"] = [type(e).__name__, str(e)]
    rec.update(rng_after=describe(rng), env_steps=planner.env_steps, last_is_result=out is not None and planner.last is out,
               last_is_set=planner.last is not None, owns_device_tree=planner.owns_device_tree())
    return rec


def visit_log(planner):
    """What MCTS logged for get_visits: the step events and, of every plan, all but the model's spec."""
    out = []
    for kind, e in getattr(planner, "_visit_log", []):
        out.append([kind, describe({k: v for k, v in e.items() if k != "spec"}) if kind == "plan" else describe(e)])
    return out


def batch_case(make_agent, make_env, n, fail=None, calls=1, between=None, root_states=None, **plan_kw):
    """``calls`` plan_batch calls of ``n`` roots on one planner; ``between(ctx, planner, k)`` runs before call k > 0."""
    def case():
        ctx = Ctx(fail)
        env = make_env()
        agent = make_agent(env)
        planner = with_stand_in(agent, ctx)
        state = agent.joint_env() if hasattr(agent, "joint_env") else env       # (the robust planner plans on its JointEnv)
        roots = list(range(1, n + 1)) if root_states is None else root_states
        records = []
        for k in range(calls):
            kw = dict(plan_kw)
            if k > 0 and between is not None:
                kw.update(between(ctx, planner, k) or {})
            rng = rng_records(n)
            records.append(plan_record(ctx, planner, lambda: planner.plan_batch(state, roots, [k] * n, rng_states=rng, **kw), rng))
        return dict(plans=records, visit_log=visit_log(planner), gap=getattr(planner, "_visit_gap", None)), ctx
    return case


def construction_case(make_agent, make_env):
    def case():
        return dict(planner=type(make_agent(make_env()).planner).__name__), Ctx()
    return case


def per_episode_case(make_agent, make_envs, fail=None, **evaluation_kw):
    """Two lock-steps of three environments through PerEpisodeEvaluation.run(): every ``_plan`` and what it returns."""
    def case():
        ctx = Ctx(fail)
        envs = make_envs()
        agent = make_agent(envs[0])
        if hasattr(agent, "planner"):
            with_stand_in(agent, ctx)
        ev = PerEpisodeEvaluation(envs, agent, sim_seed=5, max_steps=2, **evaluation_kw)
        assert ev.ctx is ctx
        steps, inner = [], ev._plan

        def recorded_plan(live, states, steps_):
            first, env_steps = inner(live, states, steps_)
            steps.append(dict(live=list(live), first=describe(first), env_steps=env_steps, rng=describe(ev.rng)))
            return first, env_steps
        ev._plan = recorded_plan
        rec = dict(kind=ev.kind, subtree=ev.subtree)
        try:
            out = ev.run()
            rec["result"] = describe({k: out[k] for k in ("returns", "lengths", "actions", "planner_env_steps", "uploads")})
        except Exception as e:     # noqa: BLE001
            rec["error"] = [type(e).__name__, str(e)]
        rec.update(lock_steps=steps, rng_after=describe(ev.rng))
        if hasattr(agent, "planner"):
            p = agent.planner
            rec.update(env_steps=p.env_steps, last_is_set=p.last is not None, owns_device_tree=p.owns_device_tree())
        return rec, ctx
    return case


def three(make_env):
    return lambda: [make_env(shift=i, state=(0, 3, 7)[i]) for i in range(3)]


def vi_agent(env):
    agent = object.__new__(ValueIterationAgent)        # (its constructor solves the template's MDP: not this loop's call)
    agent.config = dict(gamma=0.9, iterations=5)
    return agent


def agent_of(cls, config):
    return lambda env: cls(env, copy.deepcopy(config))


def lose_tree(ctx, planner, k):
    ctx._tree_owner = None


def keep(labels):
    return lambda ctx, planner, k: dict(keep_actions=labels)


def keep_after_losing(labels):
    def between(ctx, planner, k):
        ctx._tree_owner = None
        return dict(keep_actions=labels)
    return between


def step_subtree(ctx, planner, k):
    planner.step_by_subtree(1)


def step_subtree_then_lose(ctx, planner, k):
    planner.step_by_subtree(1)
    ctx._tree_owner = None


def describe_tree(root):
    """Breadth first: every node's class, its key among its parent's children and what build_gape_tree gave it."""
    out, queue = [], [(None, root)]
    while queue:
        key, node = queue.pop(0)
        out.append([type(node).__name__, describe(key)] + [describe(getattr(node, k, "-")) for k in (
            "count", "value_upper", "value_lower", "depth", "state", "observation", "done", "cumulative_reward", "mu_ucb", "mu_lcb")]
            + [node.parent is None or node.parent.children[key] is node, node.planner is not None])
        queue.extend(node.children.items())
    return out


def export_tree(ctx, planner, k):
    ctx.calls.append(["export_tree", describe_tree(planner.export_tree(0))])


def nan_initial_value(make_agent):
    def make(env):
        agent = make_agent(env)
        agent.planner._value_init[1] = np.nan
        return agent
    return make


def policy_source_agent(env):
    agent = MCTSAgent(env, dict(UCT))
    n_actions = env.action_space.n
    prior = (np.arange(S * n_actions).reshape(S, n_actions) % 5 + 1.0)
    prior /= prior.sum(axis=1, keepdims=True)
    rollout = np.full((S, n_actions), 1.0 / n_actions)
    agent.planner.policy_source = lambda state, model: (prior, rollout)
    return agent


OPD, ROPD = agent_of(DeterministicPlannerAgent, dict(budget=7, gamma=0.8)), agent_of(DiscreteRobustPlannerAgent, robust_config())
SAOPD = agent_of(StateAwarePlannerAgent, dict(budget=7, gamma=0.8))
RANGE, KEY, OTHER =native.ERR_REWARD_RANGE, native.ERR_OLOP_KEY, native.ERR_ARG
CASES = {}
for _n in (1, 3):
    CASES["opd_{}".format(_n)] = batch_case(OPD, plain_env, _n)
    CASES["opd_masked_{}".format(_n)] = batch_case(OPD, masked_env, _n)
    CASES["ropd_{}".format(_n)] = batch_case(ROPD, plain_env, _n)
    CASES["olop_kl_{}".format(_n)] = batch_case(agent_of(OLOPAgent, OLOP_KL), plain_env, _n)
    CASES["olop_hoeffding_{}".format(_n)] = batch_case(agent_of(OLOPAgent, OLOP_HOEFFDING), plain_env, _n)
    CASES["brue_{}".format(_n)] = batch_case(agent_of(BRUEAgent, BRUE_CFG), plain_env, _n)
    CASES["mcts_flat_{}".format(_n)] = batch_case(agent_of(MCTSAgent, UCT), plain_env, _n)
    CASES["mcts_restricted_{}".format(_n)] = batch_case(agent_of(MCTSAgent, UCT), masked_env, _n, calls=2)
CASES.update({
    "ropd_joint_states": batch_case(ROPD, plain_env, 3, root_states=[[1, 2], [3, 4], [5, 6]]),
    "olop_kl_uniform": batch_case(agent_of(OLOPAgent, dict(OLOP_KL, continuation_type="uniform")), plain_env, 3),
    "olop_kl_local_time": batch_case(agent_of(OLOPAgent, dict(OLOP_KL, upper_bound=dict(OLOP_KL["upper_bound"], time="local"))),
                                     plain_env, 3),
    "olop_kl_unknown_time": batch_case(agent_of(OLOPAgent, dict(OLOP_KL, upper_bound=dict(OLOP_KL["upper_bound"], time="never"))),
                                       plain_env, 1),
    "olop_hoeffding_uniform": batch_case(agent_of(OLOPAgent, dict(OLOP_HOEFFDING, continuation_type="uniform")), plain_env, 3),
    "olop_kl_masked_fixed": batch_case(agent_of(OLOPAgent, OLOP_KL), masked_env, 3),
    # every answer a planner maps to an exception (and one it does not), the second call of two so that what the first left shows
    "opd_reward_range": batch_case(OPD, plain_env, 3, dict(call=1, root=1, status=RANGE), calls=2),
    "opd_other_status": batch_case(OPD, plain_env, 3, dict(call=0, root=1, status=OTHER)),
    "opd_gamma_one": batch_case(agent_of(DeterministicPlannerAgent, dict(budget=7, gamma=1)), plain_env, 3),
    "opd_gamma_one_small_budget": batch_case(agent_of(DeterministicPlannerAgent, dict(budget=2, gamma=1)), plain_env, 3),
    "ropd_reward_range": batch_case(ROPD, plain_env, 3, dict(call=1, root=2, status=RANGE), calls=2),
    "ropd_other_status": batch_case(ROPD, plain_env, 3, dict(call=0, root=1, status=OTHER)),
    "ropd_gamma_one": batch_case(agent_of(DiscreteRobustPlannerAgent, robust_config(gamma=1)), plain_env, 3),
    "ropd_gamma_one_small_budget": batch_case(agent_of(DiscreteRobustPlannerAgent, robust_config(gamma=1, budget=2)), plain_env, 3),
    "olop_key": batch_case(agent_of(OLOPAgent, OLOP_KL), plain_env, 3, dict(call=1, root=1, status=KEY), calls=2),
    "olop_reward_range": batch_case(agent_of(OLOPAgent, OLOP_KL), plain_env, 3, dict(call=1, root=0, status=RANGE), calls=2),
    "olop_other_status": batch_case(agent_of(OLOPAgent, OLOP_HOEFFDING), plain_env, 3, dict(call=0, root=2, status=OTHER)),
    "olop_range_before_key": batch_case(agent_of(OLOPAgent, OLOP_KL), plain_env, 3, dict(call=0, root=0, status=RANGE)),
    "olop_gamma_one": construction_case(agent_of(OLOPAgent, dict(OLOP_KL, gamma=1)), plain_env),
    "brue_negative_plan": batch_case(agent_of(BRUEAgent, BRUE_CFG), plain_env, 3, dict(call=1, root=1, negative=True), calls=2),
    "brue_other_status": batch_case(agent_of(BRUEAgent, BRUE_CFG), plain_env, 3, dict(call=0, root=1, status=OTHER)),
    "brue_gamma_one": batch_case(agent_of(BRUEAgent, dict(BRUE_CFG, gamma=1)), plain_env, 3),
    # MCTS.plan_batch: the policy forms and what becomes of the kept trees
    "mcts_policy_source": batch_case(policy_source_agent, plain_env, 3, calls=2),
    "mcts_policy_source_restricted": batch_case(policy_source_agent, masked_env, 3),
    "mcts_preference_restricted": batch_case(agent_of(MCTSAgent, dict(UCT, prior_policy=dict(type="preference", action=1, ratio=3),
                                                                      rollout_policy=dict(type="random"))), masked_env, 3),
    "mcts_stochastic_open": batch_case(agent_of(MCTSAgent, UCT), stochastic_env, 3),
    "mcts_stochastic_closed": batch_case(agent_of(MCTSAgent, dict(UCT, closed_loop=True)), stochastic_env, 3),
    "mcts_stochastic_env_rng": batch_case(agent_of(MCTSAgent, UCT), stochastic_env, 3, env_rng_states=rng_records(3) + np.uint64(9)),
    "mcts_loop_form": batch_case(agent_of(MCTSAgent, UCT), functools.partial(masked_env, WIDE), 3, calls=2),
    "mcts_wide_flat": batch_case(agent_of(MCTSAgent, UCT), functools.partial(plain_env, n_actions=WIDE), 3),
    "mcts_keep_owned": batch_case(agent_of(MCTSAgent, UCT), plain_env, 3, calls=2, between=keep([0, 1, 2])),
    "mcts_keep_not_owned": batch_case(agent_of(MCTSAgent, UCT), plain_env, 3, calls=2, between=keep_after_losing([0, 1, 2])),
    "mcts_keep_restricted_owned": batch_case(agent_of(MCTSAgent, UCT), masked_env, 3, calls=2, between=keep([1, 1, 1])),
    "mcts_keep_stochastic_owned": batch_case(agent_of(MCTSAgent, UCT), stochastic_env, 3, calls=2, between=keep([0, 1, 2])),
    "mcts_keep_stochastic_not_owned": batch_case(agent_of(MCTSAgent, UCT), stochastic_env, 3, calls=2,
                                                 between=keep_after_losing([0, 1, 2])),
    "mcts_keep_stochastic_closed": batch_case(agent_of(MCTSAgent, dict(UCT, closed_loop=True)), stochastic_env, 3, calls=2,
                                              between=keep([0, 1, 2])),
    "mcts_keep_loop_form_owned": batch_case(agent_of(MCTSAgent, UCT), functools.partial(masked_env, WIDE), 3, calls=2,
                                            between=keep([1, 1, 1])),
    "mcts_armed": batch_case(agent_of(MCTSAgent, dict(UCT, step_strategy="subtree")), plain_env, 1, calls=3, between=step_subtree),
    "mcts_armed_tree_lost": batch_case(agent_of(MCTSAgent, dict(UCT, step_strategy="subtree")), plain_env, 1, calls=2,
                                       between=step_subtree_then_lose),
    "mcts_armed_stochastic": batch_case(agent_of(MCTSAgent, dict(UCT, step_strategy="subtree")), stochastic_env, 1, calls=2,
                                        between=step_subtree),
    "mcts_armed_stochastic_tree_lost": batch_case(agent_of(MCTSAgent, dict(UCT, step_strategy="subtree")), stochastic_env, 1,
                                                  calls=2, between=step_subtree_then_lose),
    "mcts_subtree_after_three_roots": batch_case(agent_of(MCTSAgent, dict(UCT, step_strategy="subtree")), plain_env, 3, calls=2,
                                                 between=step_subtree),
    # PerEpisodeEvaluation._plan, two lock-steps of three environments
    "each_vi": per_episode_case(vi_agent, three(plain_env)),
    "each_uct_flat": per_episode_case(agent_of(MCTSAgent, UCT), three(plain_env)),
    "each_uct_restricted": per_episode_case(agent_of(MCTSAgent, UCT), three(masked_env)),
    "each_uct_subtree": per_episode_case(agent_of(MCTSAgent, dict(UCT, step_strategy="subtree")), three(plain_env)),
    "each_uct_subtree_restricted": per_episode_case(agent_of(MCTSAgent, dict(UCT, step_strategy="subtree")), three(masked_env)),
    "each_opd": per_episode_case(OPD, three(plain_env)),
    "each_opd_masked": per_episode_case(OPD, three(masked_env)),
    "each_ropd": per_episode_case(ROPD, three(plain_env)),
    "each_olop_kl": per_episode_case(agent_of(OLOPAgent, OLOP_KL), three(plain_env)),
    "each_olop_kl_uniform": per_episode_case(agent_of(OLOPAgent, dict(OLOP_KL, continuation_type="uniform")), three(masked_env)),
    "each_olop_hoeffding": per_episode_case(agent_of(OLOPAgent, OLOP_HOEFFDING), three(plain_env)),
    "each_brue": per_episode_case(agent_of(BRUEAgent, BRUE_CFG), three(plain_env)),
    "each_opd_reward_range": per_episode_case(OPD, three(plain_env), dict(call=1, root=1, status=RANGE)),
    "each_opd_other_status": per_episode_case(OPD, three(plain_env), dict(call=1, root=1, status=OTHER)),
    # the state-aware planner has the kind of the optimistic one it subclasses: an OPD plan, OPD's reading of its statuses
    "each_state_aware": per_episode_case(SAOPD, three(plain_env)),
    "each_state_aware_reward_range": per_episode_case(SAOPD, three(plain_env), dict(call=1, root=1, status=RANGE)),
    "each_state_aware_other_status": per_episode_case(SAOPD, three(plain_env), dict(call=1, root=1, status=OTHER)),
    "each_state_aware_alloc_status": per_episode_case(SAOPD, three(plain_env), dict(call=0, root=2, status=native.MP_ERR_ALLOC)),
    "each_opd_gamma_one": per_episode_case(agent_of(DeterministicPlannerAgent, dict(budget=7, gamma=1)), three(plain_env)),
    "each_ropd_reward_range": per_episode_case(ROPD, three(plain_env), dict(call=1, root=0, status=RANGE)),
    "each_ropd_gamma_one": per_episode_case(agent_of(DiscreteRobustPlannerAgent, robust_config(gamma=1)), three(plain_env)),
    "each_olop_key": per_episode_case(agent_of(OLOPAgent, OLOP_KL), three(plain_env), dict(call=1, root=2, status=KEY)),
    "each_olop_reward_range": per_episode_case(agent_of(OLOPAgent, OLOP_KL), three(plain_env), dict(call=1, root=1, status=RANGE)),
    "each_olop_other_status": per_episode_case(agent_of(OLOPAgent, OLOP_KL), three(plain_env), dict(call=0, root=1, status=OTHER)),
    "each_brue_negative_plan": per_episode_case(agent_of(BRUEAgent, BRUE_CFG), three(plain_env), dict(call=1, root=1, negative=True)),
})


def gape_cases():
    """MDPGapEAgent on deterministic tables and StochasticMDPGapEAgent on a dense and a sparse model: what reaches the binding,
    every status either maps to an exception, every refusal that comes after the generator records were made."""
    cases = {}
    no_arm, holders = native.ERR_GAPE_NO_CHALLENGER, native.ERR_GAPE_PLACEHOLDERS
    for tag, cls, cfg, envs in (
            ("gape", MDPGapEAgent, GAPE_CFG, dict(plain=plain_env, masked=masked_env, ordered=ordered_env)),
            ("gape_stoch", StochasticMDPGapEAgent, GAPE_STOCH_CFG, dict(
                plain=stochastic_env, sparse=functools.partial(stochastic_env, "sparse"), table=plain_env,
                ordered=functools.partial(stochastic_env, ordered=True),
                sparse_ordered=functools.partial(stochastic_env, "sparse", ordered=True)))):
        agent = agent_of(cls, cfg)
        first = envs["plain"]

        def with_config(_cls=cls, _cfg=cfg, **kw):
            return agent_of(_cls, dict(_cfg, **kw))
        for n in (1, 3):
            cases["{}_{}".format(tag, n)] = batch_case(agent, first, n)
        for name, make_env in envs.items():
            if name != "plain":
                cases["{}_{}".format(tag, name)] = batch_case(agent, make_env, 3)
        for name, status in (("no_challenger", no_arm), ("empty_choice", OTHER), ("reward_range", RANGE), ("placeholders", holders)):
            if tag == "gape_stoch" or status != holders:
                cases["{}_{}".format(tag, name)] = batch_case(agent, first, 3, dict(call=1, root=1, status=status), calls=2)
        cases[tag + "_status_ordered"] = batch_case(agent, envs["ordered"], 3, dict(call=0, root=2, status=no_arm))
        cases[tag + "_fixed_continuation"] = batch_case(with_config(continuation_type="zero"), first, 3)
        cases[tag + "_threshold_raises"] = batch_case(with_config(**gape_bound(threshold="1/(count - 2)")), first, 3, calls=2)
        cases[tag + "_threshold_not_finite"] = batch_case(with_config(**gape_bound(threshold="np.inf if count == 3 else 1.0")), first, 3)
        cases[tag + "_initial_value_not_finite"] = batch_case(nan_initial_value(agent), first, 3)
        cases[tag + "_accuracy_not_finite"] = batch_case(with_config(accuracy=float("nan")), first, 3)
        cases[tag + "_other_bound"] = batch_case(with_config(**gape_bound(type="hoeffding")), first, 3)
        cases[tag + "_subtree"] = batch_case(with_config(step_strategy="subtree"), first, 3)
        cases[tag + "_export_tree"] = batch_case(agent, first, 3, calls=2, between=export_tree)
        cases[tag + "_export_tree_ordered"] = batch_case(agent, envs["ordered"], 3, calls=2, between=export_tree)
        cases[tag + "_own_records"] = batch_case_without_records(agent, first, 3)
    cases.update({
        "gape_two_next_states": batch_case(agent_of(MDPGapEAgent, GAPE_STOCH_CFG), plain_env, 3),
        "gape_stochastic_env": batch_case(agent_of(MDPGapEAgent, GAPE_CFG), stochastic_env, 3),
        "gape_stoch_transition_raises": batch_case(agent_of(StochasticMDPGapEAgent, dict(
            GAPE_STOCH_CFG, **gape_bound(transition_threshold="1/(count - 2)"))), stochastic_env, 3, calls=2),
        "gape_stoch_both_raise": batch_case(agent_of(StochasticMDPGapEAgent, dict(
            GAPE_STOCH_CFG, **gape_bound(threshold="1/(count - 2)", transition_threshold="1/(count - 2)"))), stochastic_env, 3),
        "gape_stoch_transition_not_finite": batch_case(agent_of(StochasticMDPGapEAgent, dict(
            GAPE_STOCH_CFG, **gape_bound(transition_threshold="-np.inf if count == 2 else 1.0"))), stochastic_env, 3),
        "gape_stoch_env_rng": batch_case(agent_of(StochasticMDPGapEAgent, GAPE_STOCH_CFG), stochastic_env, 3,
                                         env_rng_states=rng_records(3) + np.uint64(9)),
        "gape_stoch_33_next_states": batch_case(agent_of(StochasticMDPGapEAgent, dict(GAPE_CFG, max_next_states_count=33)),
                                                stochastic_env, 3),
        "gape_stoch_no_next_state": batch_case(agent_of(StochasticMDPGapEAgent, dict(GAPE_CFG, max_next_states_count=0)),
                                               stochastic_env, 3),
        "gape_stoch_half_a_next_state": batch_case(agent_of(StochasticMDPGapEAgent, dict(GAPE_CFG, max_next_states_count=1.5)),
                                                   stochastic_env, 3),
        "gape_stoch_32_next_states": batch_case(agent_of(StochasticMDPGapEAgent, dict(GAPE_CFG, max_next_states_count=32.0)),
                                                stochastic_env, 1),
        "each_gape": per_episode_case(agent_of(MDPGapEAgent, GAPE_CFG), three(plain_env), kind="gape"),
        "each_gape_masked": per_episode_case(agent_of(MDPGapEAgent, GAPE_CFG), three(masked_env), kind="gape"),
        "each_gape_ordered": per_episode_case(agent_of(MDPGapEAgent, GAPE_CFG), three(ordered_env), kind="gape"),
        "each_gape_unasked": per_episode_case(agent_of(MDPGapEAgent, GAPE_CFG), three(plain_env)),
        "each_gape_no_challenger": per_episode_case(agent_of(MDPGapEAgent, GAPE_CFG), three(plain_env),
                                                    dict(call=1, root=1, status=no_arm), kind="gape"),
        "each_gape_reward_range": per_episode_case(agent_of(MDPGapEAgent, GAPE_CFG), three(plain_env),
                                                   dict(call=1, root=2, status=RANGE), kind="gape"),
        "each_gape_threshold_raises": per_episode_case(agent_of(MDPGapEAgent, dict(GAPE_CFG, **gape_bound(threshold="1/(count - 2)"))),
                                                       three(plain_env), kind="gape"),
        "each_gape_stoch_refused": per_episode_case(agent_of(StochasticMDPGapEAgent, GAPE_STOCH_CFG), three(plain_env), kind="gape"),
    })
    return cases


def batch_case_without_records(make_agent, make_env, n):
    """One plan_batch that is handed no generator records: the planner makes its own (and they come back in the result)."""
    def case():
        ctx = Ctx()
        env = make_env()
        planner = with_stand_in(make_agent(env), ctx)
        rng = np.zeros(0, np.uint64)
        return dict(plans=[plan_record(ctx, planner, lambda: planner.plan_batch(env, list(range(1, n + 1))), rng)]), ctx
    return case


CASES.update(gape_cases())

GBOPD_CFG = dict(budget=7, gamma=0.8, accuracy=0.1, sampling_timeout=3)
GBOP_CFG = dict(budget=8, episodes=2, horizon=3, gamma=0.8, accuracy=0.1, sampling_timeout=2, max_next_states_count=2,
                upper_bound=dict(type="kullback-leibler", time="global", threshold="0*np.log(time)",
                                 transition_threshold="0.1*np.log(time) + count"))
KEPT_GRAPH = "mp_plan: the model's tables or action sets changed under a kept graph (built on the previous tables)"


def graph_case(make_agent, make_env, sizes=(3,), fail=None, between=None, defer=False):
    """One plan_batch per entry of ``sizes`` (that many roots) on one graph-based planner; ``between(ctx, planner, k)`` runs
    before call k > 0.  Recorded beside plan_record's: the reference's plan of every root where the planner reads one out of a
    result (``_plan_of``) and the counts the threshold strings were evaluated for."""
    def case():
        ctx = Ctx(fail)
        env = make_env()
        planner = with_stand_in(make_agent(env), ctx)
        if defer:
            planner.defer_errors = True
        records = []
        for k, n in enumerate(sizes):
            if k > 0 and between is not None:
                between(ctx, planner, k)
            rng = rng_records(n)
            rec = plan_record(ctx, planner, lambda: planner.plan_batch(env, list(range(1, n + 1)), [k] * n, rng_states=rng), rng)
            if "result" in rec and hasattr(planner, "_plan_of"):
                rec["plan_of"] = [planner._plan_of(planner.last, i) for i in range(n)]
            if hasattr(planner, "tables"):
                rec["evaluations"] = planner.tables.evaluations
            records.append(rec)
        return dict(plans=records), ctx
    return case


def forget(ctx, planner, k):
    planner.forget()


def plan_on_one_mdp_per_root(make_agent, make_env):
    def case():
        ctx = Ctx()
        env = make_env()
        planner = with_stand_in(make_agent(env), ctx)
        rng = rng_records(2)
        return dict(plans=[plan_record(ctx, planner, lambda: planner.plan_on(planner.model_for(env), [1, 2], None, rng,
                                                                             model_index=[0, 1]), rng)]), ctx
    return case


def graph_cases():
    """GraphBasedPlanner (GBOP-D) and StochasticGraphBasedPlanner (GBOP): the handle they keep, what reaches the binding, every
    status with the exception it maps to and ``planner.env_steps`` afterwards (GBOP adds the steps before it raises, GBOP-D only
    when it does not raise)."""
    from rl_agents_amd.agents.tree_search.graph_based import GraphBasedPlannerAgent
    from rl_agents_amd.gbop import StochasticGraphBasedPlannerAgent
    cases = {}
    statuses = dict(alloc=native.MP_ERR_ALLOC, no_action=native.MP_ERR_GBOPD_NO_ACTION, diverged=native.MP_ERR_GBOPD_DIVERGED,
                    other=OTHER)
    for tag, cls, cfg, first, ordered, more in (
            ("gbopd", GraphBasedPlannerAgent, GBOPD_CFG, plain_env, ordered_env, {}),
            ("gbop", StochasticGraphBasedPlannerAgent, GBOP_CFG, stochastic_env, functools.partial(stochastic_env, ordered=True),
             dict(placeholders=native.ERR_GBOP_PLACEHOLDERS, reward_threshold=native.ERR_GBOP_REWARD_THRESHOLD,
                  choice_p=native.ERR_GBOP_CHOICE_P))):
        agent = agent_of(cls, cfg)
        cases[tag + "_kept_handle"] = graph_case(agent, first, sizes=(3, 3, 2, 2), between=lambda ctx, planner, k: (
            planner.forget() if k == 3 else None))
        cases[tag + "_one_root"] = graph_case(agent, first, sizes=(1,))
        cases[tag + "_ordered"] = graph_case(agent, ordered, sizes=(3,))
        cases[tag + "_masked_table"] = graph_case(agent, masked_env, sizes=(3,))
        cases[tag + "_defer_errors"] = graph_case(agent, first, sizes=(3, 3), fail=dict(call=1, root=1, set=dict(status=OTHER)),
                                                  defer=True)
        for name, status in dict(statuses, **more).items():
            cases["{}_status_{}".format(tag, name)] = graph_case(agent, first, sizes=(3, 3),
                                                                 fail=dict(call=1, root=1, set=dict(status=status)))
        cases[tag + "_tables_changed"] = graph_case(agent, first, sizes=(3, 3), fail=dict(call=1, error=KEPT_GRAPH))
        cases[tag + "_other_native_error"] = graph_case(agent, first, sizes=(3,), fail=dict(call=0, error="mp_plan: out of memory"))
        cases["each_" + tag] = per_episode_case(agent, three(plain_env))
    gbop = functools.partial(agent_of, StochasticGraphBasedPlannerAgent)
    cases.update({
        "gbop_table": graph_case(gbop(GBOP_CFG), plain_env, sizes=(3,)),
        "gbop_sparse": graph_case(gbop(GBOP_CFG), functools.partial(stochastic_env, "sparse"), sizes=(3,)),
        "gbop_one_mdp_per_root": plan_on_one_mdp_per_root(gbop(GBOP_CFG), stochastic_env),
        "gbop_other_bound": graph_case(gbop(dict(GBOP_CFG, upper_bound=dict(GBOP_CFG["upper_bound"], type="hoeffding"))),
                                       stochastic_env),
        "gbop_no_next_state": graph_case(gbop(dict(GBOP_CFG, max_next_states_count=0)), stochastic_env),
        "gbop_33_next_states": graph_case(gbop(dict(GBOP_CFG, max_next_states_count=33)), stochastic_env),
        "gbop_half_a_next_state": graph_case(gbop(dict(GBOP_CFG, max_next_states_count=1.5)), stochastic_env),
        "gbop_next_states_changed": graph_case(gbop(GBOP_CFG), stochastic_env, sizes=(3, 3), between=lambda ctx, planner, k: (
            planner.config.update(max_next_states_count=3))),
        "gbop_threshold_raises": graph_case(gbop(dict(GBOP_CFG, upper_bound=dict(
            GBOP_CFG["upper_bound"], transition_threshold="1/(count - 8)"))), stochastic_env, sizes=(3, 3)),
        "gbop_plan_len_0": graph_case(gbop(GBOP_CFG), stochastic_env, fail=dict(call=0, root=1, set=dict(plan_len=0, plans=-1))),
        "gbop_plan_len_2": graph_case(gbop(GBOP_CFG), stochastic_env, fail=dict(call=0, root=1, set=dict(plan_len=2, key=7))),
        "gbop_plan_len_2_placeholder": graph_case(gbop(GBOP_CFG), stochastic_env,
                                                  fail=dict(call=0, root=2, set=dict(plan_len=2, key=-2))),
    })
    return cases


CASES.update(graph_cases())


def run_case(name, mp):
    mp.setattr(runtime, "get_context", lambda *a, **k: Ctx.current)
    mp.setattr(native, "seed_sequence_states", lambda entropy, first_key, count: rng_records(count) + np.uint64(first_key))
    mp.setattr(native, "GraphBasedPlanners", GraphPlanners)
    mp.setattr(native, "StochasticGraphBasedPlanners", StochasticGraphPlanners)
    log = Log()
    root = logging.getLogger("rl_agents_amd")
    level = root.level
    root.addHandler(log)
    root.setLevel(logging.DEBUG)
    try:
        rec, ctx = CASES[name]()
    except Exception as e:     # noqa: BLE001 - a case that cannot be built records why
        rec, ctx = dict(error=[type(e).__name__, str(e)]), Ctx()
    finally:
        root.removeHandler(log)
        root.setLevel(level)
        mp.undo()
    rec["calls"], rec["log"] = ctx.calls, log.lines
    return json.loads(json.dumps(rec))


@functools.lru_cache(maxsize=None)
def _expected():
    with open(RECORD) as f:
        return json.load(f)


def test_record_holds_exactly_the_cases():
    assert sorted(_expected()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_planner_calls(name, monkeypatch):
    expected = _expected()[name]
    got = run_case(name, monkeypatch)
    for key in sorted(set(expected) | set(got)):
        assert json.dumps(got.get(key), sort_keys=True) == json.dumps(expected.get(key), sort_keys=True), key


# ---- what PerEpisodeEvaluation makes of every planner class: written out by hand from the isinstance ladder this table replaced
NO_KIND = "per-episode tables: this loop has no kind that plans {} on one model per episode, and would run the optimistic " \
          "planner in its place"
KEPT_STATE = "per-episode tables: {} keeps its planner state (graph, bounds, state values) from plan to plan, and a kept state " \
             "was built on the previous step's table"
KINDS = {
    "OptimisticDeterministicPlanner": "opd",
    "StateAwarePlanner": "opd",                 # (a subclass of the optimistic planner without an opt-out: the ladder's fallback)
    "DiscreteRobustPlanner": "ropd",
    "OLOP": "olop",
    "StochasticOLOP": "olop",
    "BRUE": "brue",
    "MCTS": "uct",
    "MDPGapE": NotImplementedError(NO_KIND.format("MDPGapE")),
    "SparseSampling": NotImplementedError(NO_KIND.format("SparseSampling")),
    "GraphBasedPlanner": NotImplementedError(KEPT_STATE.format("GraphBasedPlanner")),
}


def planner_classes():
    """Every subclass of AbstractPlanner that a module under rl_agents_amd/agents defines."""
    import importlib
    import pkgutil
    import rl_agents_amd.agents as package
    from rl_agents_amd.agents.tree_search.abstract import AbstractPlanner
    found = {}
    for info in pkgutil.walk_packages(package.__path__, package.__name__ + "."):
        module = importlib.import_module(info.name)
        for cls in vars(module).values():
            if isinstance(cls, type) and issubclass(cls, AbstractPlanner) and cls is not AbstractPlanner \
                    and cls.__module__ == module.__name__:
                found[cls.__name__] = cls
    return found


def evaluation_of(cls, **config):
    from rl_agents_amd.agents.tree_search.mcts import MCTS
    import types
    env = plain_env()
    config = dict(UCT, **config)
    flat = {"type": "random_available"}
    planner = MCTS(env, flat, flat, config) if cls is MCTS else cls(env, config)
    planner.models = Models(Ctx())
    return PerEpisodeEvaluation([plain_env(), plain_env()], types.SimpleNamespace(planner=planner, config=config))


def test_per_episode_kind_of_every_planner_class(monkeypatch):
    monkeypatch.setattr(runtime, "get_context", lambda *a, **k: Ctx.current)
    classes = planner_classes()
    assert sorted(classes) == sorted(KINDS)
    for name, expected in KINDS.items():
        if isinstance(expected, Exception):
            with pytest.raises(type(expected)) as raised:
                evaluation_of(classes[name])
            assert str(raised.value) == str(expected), name
        else:
            ev = evaluation_of(classes[name])
            assert (ev.kind, ev.subtree, ev.vi) == (expected, False, False), name
    ev = PerEpisodeEvaluation([plain_env()], vi_agent(plain_env()))
    assert (ev.kind, ev.subtree, ev.vi) == ("vi", False, True)
    kept = evaluation_of(classes["MCTS"], step_strategy="subtree")
    assert (kept.kind, kept.subtree) == ("uct", True)
    for name in ("MCTS", "OptimisticDeterministicPlanner", "DiscreteRobustPlanner"):
        with pytest.raises(NotImplementedError, match="step_strategy must be 'reset'"):
            evaluation_of(classes[name], step_strategy="subtree", closed_loop=True)


def test_device_statuses_are_read_where_a_planner_has_codes():
    """AbstractPlanner.raise_for_device_status: the live slots' statuses through the planner's own mapping; a planner without
    status codes (MCTS) touches neither buffer."""
    import torch
    classes = planner_classes()

    class Untouched(object):
        def __getitem__(self, key):
            raise AssertionError("the status buffer was read")

    def planner_of(name):
        flat = {"type": "random_available"}
        return classes[name](plain_env(), flat, flat, dict(UCT)) if name == "MCTS" else classes[name](plain_env(), dict(UCT))
    planner_of("MCTS").raise_for_device_status(Untouched(), Untouched())
    status = torch.tensor([[0, RANGE], [0, 0]], dtype=torch.int32)
    live = torch.tensor([[True, False], [True, True]])
    for name in ("OptimisticDeterministicPlanner", "DiscreteRobustPlanner", "StateAwarePlanner"):
        planner_of(name).raise_for_device_status(status, live)                   # (the failed slot is not live)
        planner_of(name).raise_for_device_status(status, torch.zeros(2, 2, dtype=torch.bool))
        with pytest.raises(ValueError, match="rewards are normalized"):
            planner_of(name).raise_for_device_status(status, torch.ones(2, 2, dtype=torch.bool))
    other = torch.tensor([[0, OTHER]], dtype=torch.int32)
    planner_of("OptimisticDeterministicPlanner").raise_for_device_status(other, torch.ones(1, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="empty sequence"):
        planner_of("StateAwarePlanner").raise_for_device_status(other, torch.ones(1, 2, dtype=torch.bool))


def record_all():
    out = {}
    for name in sorted(CASES):
        mp = pytest.MonkeyPatch()
        try:
            out[name] = run_case(name, mp)
        finally:
            mp.undo()
    return out


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_planner_calls_host.py --write   (the rl_agents_amd first on PYTHONPATH is recorded)")
    with open(RECORD, "w") as f:
        f.write("{\n" + ",\n".join("{}:{}".format(json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":")))
                                  for k, v in sorted(record_all().items())) + "\n}\n")
    print("wrote {} cases to {}".format(len(CASES), RECORD))
