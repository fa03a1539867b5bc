"""MDP-GapE with transition bounds on the host: the test-side restatement (tests/gape_stoch_restatement.py) against the
reference's own outputs (tests/golden/gape_stoch.npz and tests/golden/gape_transition.npz, bit for bit), against the
deterministic restatement at one next state, the new agent's config surface, tables and refusals, the reference's configs,
the header -- no GPU needed."""
import os
import re

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv, generators
from tests import gape_restatement as gr
from tests import gape_stoch_restatement as gs
from tests.helpers import generator_from
from tests.test_gape_host import REFERENCE_CONFIGS, NoDevice

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gape_stoch.npz")
TRANSITION = os.path.join(HERE, "golden", "gape_transition.npz")
STOCH_AGENT = "<class 'rl_agents_amd.agents.tree_search.mdp_gape.StochasticMDPGapEAgent'>"
GAPE_AGENT = "<class 'rl_agents_amd.agents.tree_search.mdp_gape.MDPGapEAgent'>"
RESTATED_ERRORS = {"placeholders": "placeholders", "reward_range": "range"}
EXACT = ("parent", "kind", "action", "depth", "count", "done", "cum")
BOUNDS = ("mu_ucb", "mu_lcb", "vu", "vl")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def names(z):
    return [str(n) for n in z["gape_stoch/names"]]


def golden_case(z, name):
    p = "gape_stoch/" + name
    return {k[len(p) + 1:]: z[k] for k in z.files if k.startswith(p + "/")}


def case_tables(case):
    n_actions = case["mdp/reward"].shape[1]
    args = (int(case["horizon"]), n_actions, float(case["confidence"]), int(case["episodes"]))
    return (gr.thresholds_by_count(str(case["threshold"]), *args),
            gs.transition_thresholds_by_count(str(case["transition_threshold"]), *args))


def restate(case, rng6=None, s0=None, observe=None, log=np.log, exp=np.exp):
    """The restatement on one golden case's inputs -> (result, the planner's generator after)."""
    gen = generator_from(case["rng_before"] if rng6 is None else rng6)
    thr, tthr = case_tables(case)
    res = gs.gape_stoch_plan(str(case["mdp/mode"]), case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"],
                             int(case["s0"]) if s0 is None else s0, int(case["episodes"]), int(case["horizon"]),
                             float(case["gamma"]), float(case["accuracy"]), thr, tthr, int(case["max_next_states_count"]),
                             str(case["continuation"]), gen, next_states=case.get("mdp/next"), available=case["available"],
                             order=case["order"], done_rule="next" if bool(case["done_on_next"]) else "source", observe=observe,
                             log=log, exp=exp)
    return res, gen


def case_env(case, s0=None):
    """The env of a golden case: its table, availability, listing order and done rule."""
    c = dict(mode=str(case["mdp/mode"]), transition=case["mdp/transition"].tolist(), reward=case["mdp/reward"].tolist(),
             terminal=case["mdp/terminal"].astype(int).tolist(), state=int(case["s0"]) if s0 is None else int(s0), max_steps=0,
             done_rule="next" if bool(case["done_on_next"]) else "source")
    if c["mode"] == "sparse":
        c["next"] = case["mdp/next"].tolist()
    available, order = case["available"], case["order"]
    if not np.array_equal(order, np.arange(len(order))):
        env = OrderedMaskedFiniteMDPEnv(dict(c, available=available.astype(int).tolist(), listing_order=[int(a) for a in order]))
    elif not available.all():
        env = MaskedFiniteMDPEnv(dict(c, available=available.astype(int).tolist()))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def case_agent(case, s0=None):
    env = case_env(case, s0)
    cfg = dict(gamma=float(case["gamma"]), episodes=int(case["episodes"]), horizon=int(case["horizon"]), budget=int(case["budget"]),
               accuracy=float(case["accuracy"]), confidence=float(case["confidence"]), continuation_type=str(case["continuation"]),
               max_next_states_count=int(case["max_next_states_count"]),
               upper_bound=dict(type="kullback-leibler", threshold=str(case["threshold"]),
                                transition_threshold=str(case["transition_threshold"])))
    agent = agent_factory(env, dict(cfg, __class__=STOCH_AGENT))
    native.generator_set_state(agent.planner.np_random, case["rng_before"])
    return env, agent


def golden_tree(case):
    return {k: case["tree/" + k] for k in EXACT + BOUNDS}


def test_restatement_equals_reference_goldens(z):
    planned = 0
    for name in names(z):
        case = golden_case(z, name)
        res, gen = restate(case)
        assert res["env_steps"] == int(case["env_steps"]), name
        assert np.array_equal(native.rng_state_from_generator(gen), case["rng_after"]), name
        if str(case["error"]):
            assert str(case["error"]) == "ValueError" and res["error"] == RESTATED_ERRORS[name], name
            continue
        assert res["error"] is None and np.array_equal(res["plan"], case["plan"]), name
        assert res["episodes_run"] == int(case["episodes_run"]), name
        tree = gs.as_bfs(res)
        for k in EXACT + BOUNDS:
            assert np.array_equal(tree[k], case["tree/" + k]), (name, k)       # numpy's own log, exp and @: bits
        planned += 1
    assert planned == 11


def test_goldens_cover_the_issue_cases(z):
    cases = {n: golden_case(z, n) for n in names(z)}
    ok = {n: c for n, c in cases.items() if not str(c["error"])}
    assert float(z["gape_stoch/margin"]) > 1e-9 and all(float(c["margin"]) > 1e-9 for c in ok.values())
    finite = REFERENCE_CONFIGS["FiniteMDPEnv/agents/mdp-gape.json"]
    for name, mode, k in (("finite_sparse_b2", "sparse", 2), ("finite_dense8_k8", "stochastic", 8), ("finite_det_k2", "deterministic", 2)):
        c = ok[name]
        assert (str(c["mdp/mode"]), int(c["max_next_states_count"])) == (mode, k), name
        assert (float(c["gamma"]), int(c["budget"]), float(c["accuracy"]), float(c["confidence"]), str(c["threshold"])) == \
            (finite["gamma"], finite["budget"], finite["accuracy"], finite["confidence"], finite["upper_bound"]["threshold"]), name
        assert str(c["transition_threshold"]) == "0.1*np.log(time)", name        # the default: the JSON's key is never read
    assert ok["finite_dense8_k8"]["mdp/reward"].shape[0] == 8
    det2 = ok["finite_det_k2"]
    assert (det2["tree/action"][det2["tree/kind"] == 0] < -1).any()              # placeholder_1 is never assigned
    assert str(ok["default_sparse_b3_k3"]["mdp/mode"]) == "sparse" and int(ok["default_sparse_b3_k3"]["max_next_states_count"]) == 3
    assert ok["default_sparse_b3_k3"]["mdp/transition"].shape[2] == 3 and str(ok["default_sparse_b3_k3"]["threshold"]) == gr.DEFAULT_THRESHOLD
    assert str(ok["det_k1"]["mdp/mode"]) == "deterministic" and int(ok["det_k1"]["max_next_states_count"]) == 1
    bad = cases["placeholders"]
    assert str(bad["error"]) == "ValueError" and "placeholder" in str(bad["message"])
    assert bad["mdp/transition"].shape[2] > int(bad["max_next_states_count"]) and int(bad["env_steps"]) > int(bad["horizon"])
    assert not bool(ok["terminal_source"]["done_on_next"]) and ok["terminal_source"]["tree/done"].any()
    assert bool(ok["terminal_next"]["done_on_next"]) and ok["terminal_next"]["tree/done"].any()
    masked = ok["masked_ordered"]
    assert not masked["available"].all() and not np.array_equal(masked["order"], np.arange(len(masked["order"])))
    assert str(ok["zeros"]["continuation"]) == "zeros" and "count" in str(ok["threshold_by_count"]["transition_threshold"])
    assert str(cases["reward_range"]["error"]) == "ValueError" and int(cases["reward_range"]["env_steps"]) > 1
    assert int(ok["early_stop"]["episodes_run"]) < int(ok["early_stop"]["episodes"])
    for name in ("finite_sparse_b2", "finite_dense8_k8", "default_sparse_b3_k3"):
        assert int(ok[name]["newton"]) > 0 and int(ok[name]["zero_mass"]) > 0, name


@pytest.mark.parametrize("name", ["det_k1", "finite_det_k2"])
def test_one_next_state_on_a_table_is_the_deterministic_restatement(z, name):
    """At K = 1 on a deterministic table the restatement gives what tests/gape_restatement.py gives, bit for bit: p_hat = [1.0]
    comes back from the isclose branch and 1.0 * u == u."""
    case = dict(golden_case(z, name), max_next_states_count=1)
    res, gen = restate(case)
    gen0 = generator_from(case["rng_before"])
    thr, _ = case_tables(case)
    det = gr.gape_plan(case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"], int(case["s0"]), int(case["episodes"]),
                       int(case["horizon"]), float(case["gamma"]), float(case["accuracy"]), thr, str(case["continuation"]), gen0,
                       available=case["available"], order=case["order"])
    assert np.array_equal(native.rng_state_from_generator(gen), native.rng_state_from_generator(gen0))
    for k in ("plan", "env_steps", "episodes_run", "best", "challenger", "parent") + gr.TREE_KEYS:
        assert np.array_equal(res[k], det[k]), k


TRANSITION_SETS = (1, 2, 3, 5, 32, "_hand")        # the lattice by width, and the hand-made points of width 4


def test_transition_restatement_equals_the_reference_lattice():
    g = np.load(TRANSITION)
    n = 0
    for K in TRANSITION_SETS:
        f, q, c = g["f%s" % K], g["q%s" % K], g["c%s" % K]
        for i in range(len(c)):
            p, its, mask = gs.max_expectation(f[i], q[i], c[i])
            assert np.array_equal(p, g["p%s" % K][i], equal_nan=True), (K, i)
            assert (its, mask) == (int(g["iterations%s" % K][i]), int(g["decisions%s" % K][i])), (K, i)
            n += 1
    flagged = sum(int(g["flag%s" % K].sum()) for K in TRANSITION_SETS)
    assert flagged <= 0.05 * n, (flagged, n)
    seen = np.bitwise_or.reduce(np.concatenate([g["decisions%s" % K] for K in TRANSITION_SETS]))
    for bit in (gs.KT_UNIFORM_Q, gs.KT_FSTAR_ABOVE, gs.KT_ZERO_MASS, gs.KT_ISCLOSE, gs.KT_NEWTON, gs.KT_CLAMP, gs.KT_BETA_ZERO,
                gs.KT_BETA_UNIFORM):
        assert seen & bit, bit
    # beta == 0 with and without its uniform fallback, at points the reference itself is stable at
    hand = g["decisions_hand"][~g["flag_hand"]]
    assert (hand & gs.KT_BETA_ZERO).all() and (hand & gs.KT_BETA_UNIFORM).any() and not (hand & gs.KT_BETA_UNIFORM).all()
    assert {float(x) for K in (1, 2, 3, 5, 32) for x in np.unique(g["c%d" % K])} == {0.0, 1e-3, 0.1, 2.0}
    # c == 0 is thin on purpose (one point per kind of f and width): most of those points are flagged, see the generator
    zero_c = sum(int((g["c%d" % K] == 0).sum()) for K in (1, 2, 3, 5, 32))
    assert 20 <= zero_c <= 30, zero_c


def test_a_raising_transition_threshold_is_raised_before_the_launch():
    """Where this differs from the reference: the string is evaluated on the host before anything is planned,
    so its exception comes with the generator as it was and no step booked; the reference reaches it at the first backup."""
    env = sparse_env()
    agent = agent_factory(env, {"__class__": STOCH_AGENT, "budget": 50, "max_next_states_count": 2,
                                "upper_bound": {"transition_threshold": "1 / (count - count)"}})
    agent.planner.models = StopAtThePlanCall()
    before = native.rng_state_from_generator(agent.planner.np_random).copy()
    with pytest.raises(ZeroDivisionError):
        agent.plan(0)
    assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), before) and agent.planner.env_steps == 0


def sparse_env(k=3, seed=3):
    env = FiniteMDPEnv(dict(generators.random_sparse(10, 3, k, seed=seed)))
    env.reset()
    return env


def test_config_surface_and_tables():
    from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapE, MDPGapEAgent, StochasticMDPGapE, StochasticMDPGapEAgent
    by_count = "0.1*np.log(time) + 0.05*np.log(1 + count) + 0*horizon*actions*confidence"
    agent = agent_factory(sparse_env(), {"__class__": STOCH_AGENT, "budget": 100, "gamma": 0.8, "max_next_states_count": 3,
                                         "upper_bound": {"transition_threshold": by_count}})
    assert isinstance(agent, StochasticMDPGapEAgent) and isinstance(agent, MDPGapEAgent)
    planner = agent.planner
    assert type(planner) is StochasticMDPGapE and isinstance(planner, MDPGapE)
    assert planner.accepts_stochastic_models and not MDPGapE.accepts_stochastic_models and planner.per_episode_kind is None
    assert planner.supports_device_loop() is False
    cfg = planner.config
    assert cfg["upper_bound"]["threshold"] == gr.DEFAULT_THRESHOLD and cfg["max_next_states_count"] == 3
    horizon, actions, confidence, time = cfg["horizon"], 3, cfg["confidence"], cfg["episodes"]  # noqa: F841
    table = planner.transition_thresholds()
    assert len(table) == cfg["episodes"] + 2
    for count in range(1, len(table) + 1):
        assert table[count - 1] == eval(by_count)
    assert np.array_equal(table, gs.transition_thresholds_by_count(by_count, horizon, actions, confidence, time))
    assert np.array_equal(planner.thresholds(), gr.thresholds_by_count(gr.DEFAULT_THRESHOLD, horizon, actions, confidence, time))
    default = agent_factory(sparse_env(), {"__class__": STOCH_AGENT, "budget": 100}).planner
    assert default.config["max_next_states_count"] == 1
    assert np.array_equal(default.transition_thresholds(), np.full(default.config["episodes"] + 2, 0.1 * np.log(default.config["episodes"])))


def test_refusals_of_the_new_agent():
    with pytest.raises(NotImplementedError, match="subtree"):
        agent_factory(sparse_env(), {"__class__": STOCH_AGENT, "step_strategy": "subtree"})
    for count, error in ((33, NotImplementedError), (0, ValueError), (-1, ValueError), (1.5, ValueError)):
        agent = agent_factory(sparse_env(), {"__class__": STOCH_AGENT, "budget": 50, "max_next_states_count": count})
        agent.planner.models = NoDevice()
        with pytest.raises(error, match="max_next_states_count"):
            agent.planner.plan_batch(sparse_env(), [0])
    agent = agent_factory(sparse_env(), {"__class__": STOCH_AGENT, "budget": 50, "upper_bound": {"type": "hoeffding"}})
    agent.planner.models = NoDevice()
    with pytest.raises(ValueError, match="only logs"):
        agent.planner.plan_batch(sparse_env(), [0])
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    agent = agent_factory(sparse_env(), {"__class__": STOCH_AGENT, "budget": 50})
    with pytest.raises(NotImplementedError, match="one model per episode"):
        PerEpisodeEvaluation([sparse_env(), sparse_env()], agent)


def test_the_old_agent_still_refuses():
    env = sparse_env()
    with pytest.raises(TypeError, match="deterministic"):
        agent_factory(env, {"__class__": GAPE_AGENT, "budget": 50}).planner.plan_batch(env, [0])
    det = FiniteMDPEnv(dict(generators.random_deterministic(10, 3, seed=1)))
    agent = agent_factory(det, {"__class__": GAPE_AGENT, "budget": 50, "max_next_states_count": 2})
    agent.planner.models = NoDevice()
    with pytest.raises(NotImplementedError, match="placeholder"):
        agent.planner.plan_batch(det, [0])


class PlanCallReached(Exception):
    pass


class StopAtThePlanCall(object):
    """Stands where the model cache is: hands out a model description, and its context's plan call is the end of the test."""

    class Model(object):
        A, mode, action_order = 3, native.MODE_SPARSE, None

        def set_available(self, *a):
            pass

        def set_episode_rules(self, *a):
            pass

    class Ctx(object):
        _tree_owner = None

        def gape_plan_stochastic(self, model, roots, episodes, horizon, count, *rest):
            raise PlanCallReached(count, len(rest[5]), len(rest[6]))      # the two threshold tables

    ctx = Ctx()

    def get(self, spec):
        return self.Model()


@pytest.mark.parametrize("name", sorted(n for n in REFERENCE_CONFIGS if REFERENCE_CONFIGS[n]["max_next_states_count"] == 2))
def test_reference_configs_with_two_next_states_reach_the_plan_call(name):
    cfg = dict(REFERENCE_CONFIGS[name], __class__=STOCH_AGENT)
    env = sparse_env(k=2)
    agent = agent_factory(env, cfg)
    pc = agent.planner.config
    assert pc["max_next_states_count"] == 2 and pc["upper_bound"]["transition_threshold"] == "0.1*np.log(time)"
    assert "threshold_transition" in pc["upper_bound"]                      # the JSON's spelling rides along, unread
    agent.planner.models = StopAtThePlanCall()
    with pytest.raises(PlanCallReached) as reached:
        agent.planner.plan_batch(env, [0])
    assert reached.value.args == (2, pc["episodes"] + 2, pc["episodes"] + 2)
    # and the old agent refuses the same config
    old = agent_factory(env, dict(cfg, __class__=GAPE_AGENT))
    old.planner.models = NoDevice()
    with pytest.raises(NotImplementedError, match="placeholder"):
        old.planner.plan_batch(env, [0])


def test_header_signatures_and_library_have_the_entry_points():
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+MP_ERR_GAPE_PLACEHOLDERS\s+\(-10\)", header) and native.ERR_GAPE_PLACEHOLDERS == -10
    assert re.search(r"#define\s+MP_ABI_VERSION\s+7\b", header)
    assert re.search(r"\bconst char \*mp_gape_stoch_form_names\(void\);", header)
    lib = native.load()
    assert lib.mp_abi_version() == 7
    for symbol in ("mp_gape_plan_stochastic", "mp_gape_stoch_tree_export", "mp_selftest_gape_transition"):
        assert symbol in native.SIGNATURES and getattr(lib, symbol) is not None, symbol
        declared = re.search(r"\bint %s\(([^;]*)\);" % symbol, header).group(1)
        assert len(native.SIGNATURES[symbol][1]) == declared.count(",") + 1, symbol
    form_names = native.gape_stoch_form_names()
    assert form_names == ["gape_stoch_table", "gape_stoch_table_slots", "gape_stoch_dense", "gape_stoch_dense_slots",
                          "gape_stoch_sparse", "gape_stoch_sparse_slots"]
    for other in (native.kernel_form_names(), native.each_form_names(), native.ss_form_names(), native.olop_stoch_form_names(),
                  native.gape_form_names()):
        assert not set(form_names) & set(other)
    # the device's decision bits are the restatement's
    with open(os.path.join(HERE, "..", "rl_agents_amd", "csrc", "kl_transition.hpp")) as f:
        source = f.read()
    for name in ("KT_UNIFORM_Q", "KT_FSTAR_ABOVE", "KT_ZERO_MASS", "KT_ISCLOSE", "KT_NEWTON", "KT_CLAMP", "KT_FINAL_CLAMP",
                 "KT_BETA_ZERO", "KT_BETA_UNIFORM"):
        assert int(re.search(r"\b%s = (\d+)" % name, source).group(1)) == getattr(gs, name), name


# ---- the sweep of tests/test_gpu_gape_stoch_sweep.py: what it holds, on the restatement alone ------------------------------------
@pytest.fixture(scope="module")
def sweep():
    from tests import gape_stoch_cases as gc
    cases = [gc.sweep_case(i) for i in range(gc.N_CASES)]
    return [(case, gc.restate_case(case)) for case in cases]


def test_sweep_skips_at_most_the_cap_and_holds_what_it_is_for(sweep):
    from tests import gape_stoch_cases as gc
    plans = [(case, p) for case, restated in sweep for p in restated]
    close = sum(1 for _, p in plans if gc.margin(p[2]) <= gc.MARGIN)
    print("sweep: {} plans, {} with margin <= {}".format(len(plans), close, gc.MARGIN))
    assert len(plans) == gc.N_CASES * gc.ROOTS == 60 and close <= gc.SKIP_CAP * len(plans), close

    def some(pred):
        return any(pred(case, p[0], p[2]) for case, p in plans)

    def planned(res):
        return res["error"] is None

    for mode in gc.MODES:
        # (a table's chance node sees one next state: f_p has one entry and the Newton branch is never taken there)
        assert mode == "deterministic" or some(lambda c, r, s: str(c["mdp/mode"]) == mode and planned(r)
                                               and any(k == "transition/eps" for k, _ in s)), mode
        assert some(lambda c, r, s: str(c["mdp/mode"]) == mode and planned(r) and any(k == "transition/theta_star" for k, _ in s)), mode
    for count in (1, 2, 3, 4, 32):
        assert some(lambda c, r, s: int(c["max_next_states_count"]) == count and planned(r)), count
    assert some(lambda c, r, s: c["mdp/reward"].shape == (32, 2) and str(c["mdp/mode"]) == "stochastic" and planned(r))
    assert some(lambda c, r, s: c["mdp/reward"].shape[1] == 70 and planned(r))
    assert some(lambda c, r, s: int(c["horizon"]) == 20 and planned(r))
    assert {c["mdp/reward"].shape[1] for c, _ in plans} >= {2, 3, 4, 5} and min(c["mdp/reward"].shape[0] for c, _ in plans) == 4
    assert max(c["mdp/reward"].shape[0] for c, _ in plans) >= 28
    for on_next in (False, True):
        assert some(lambda c, r, s: bool(c["done_on_next"]) == on_next and planned(r) and r["done"].any()), on_next
    for continuation in ("uniform", "zeros"):
        assert some(lambda c, r, s: not c["available"].all() and str(c["continuation"]) == continuation and planned(r)), continuation
    assert some(lambda c, r, s: not np.array_equal(c["order"], np.arange(len(c["order"]))) and planned(r))
    assert some(lambda c, r, s: r["error"] == "placeholders" and r["env_steps"] > 0)
    assert some(lambda c, r, s: r["error"] == "one_action" and r["env_steps"] == 0)
    assert some(lambda c, r, s: planned(r) and r["episodes_run"] < int(c["episodes"]) + 2)
    assert some(lambda c, r, s: planned(r) and (r["action"][r["kind"] == 0] < -1).any())        # a placeholder left unassigned
    assert {str(c["transition_threshold"]) for c, _ in plans} == {gc.DEFAULT_TRANSITION, gc.BY_COUNT}
    assert not any(((c["mdp/reward"] == 0) | (c["mdp/reward"] == 1)).any() for c, _ in plans)


def test_margins_of_the_slots_batch_of_the_device():
    """The roots that test_more_trees_than_the_workspace_keeps (tests/test_gpu_gape_stoch_sweep.py) compares with the
    restatement, for a device of 256 compute units (8192 resident workgroups): no comparison of theirs is closer than 1e-9."""
    from tests import gape_stoch_cases as gc
    from tests.test_gpu_gape_stoch_sweep import slots_batch, slots_sample
    env, agent, case, roots, rng0 = slots_batch()
    both = gc.tables(case)
    stopped_early = 0
    for i in slots_sample(len(roots), 256 * 32):
        res, _, seen = gc.restate_plan(case, int(roots[i]), rng0[i], both)
        assert res["error"] is None and gc.margin(seen) > gc.MARGIN, (i, gc.margin(seen))
        stopped_early += res["episodes_run"] < int(case["episodes"]) + 2
    print("slots sample: {} of 8 stop early".format(stopped_early))
