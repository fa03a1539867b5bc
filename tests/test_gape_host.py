"""MDP-GapE on the host: the test-side restatement against the reference's own outputs (tests/golden/gape.npz, bit for bit, and
again with a jittered ``log``), the threshold table, the refusals of MDPGapEAgent, the reference's configs, the header; what the
sweep of tests/test_gpu_gape_sweep.py contains (tests/gape_cases.py), its share of plans too close to call and the margins of
the roots the batch tests of tests/test_gpu_gape.py compare -- no GPU needed."""
import json
import os
import re

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, generators
from tests import gape_cases as gc
from tests import gape_restatement as gr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gape.npz")
GAPE_AGENT = "<class 'rl_agents_amd.agents.tree_search.mdp_gape.MDPGapEAgent'>"
ERRORS = {"ValueError": ValueError, "ZeroDivisionError": ZeroDivisionError}
# the reference's four MDPGapEAgent configs (scripts/configs/*/agents), as they are
with open(os.path.join(HERE, "golden", "gape_reference_configs.json")) as _f:
    REFERENCE_CONFIGS = json.load(_f)


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def names(z):
    return [str(n) for n in z["gape/names"]]


def golden_case(z, name):
    p = "gape/" + name
    return {k[len(p) + 1:]: z[k] for k in z.files if k.startswith(p + "/")}


def generator_from(state6):
    gen = np.random.Generator(np.random.PCG64(0))
    native.generator_set_state(gen, state6)
    return gen


def case_thresholds(case):
    return gr.thresholds_by_count(str(case["threshold"]), int(case["horizon"]), case["mdp/reward"].shape[1],
                                  float(case["confidence"]), int(case["episodes"]))


def restate(case, log=np.log, rng6=None, s0=None):
    """The restatement on one golden case's inputs -> (result, generator after); the threshold's own exception passes."""
    gen = generator_from(case["rng_before"] if rng6 is None else rng6)
    res = gr.gape_plan(case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"], int(case["s0"]) if s0 is None else s0,
                       int(case["episodes"]), int(case["horizon"]), float(case["gamma"]), float(case["accuracy"]),
                       case_thresholds(case), str(case["continuation"]), gen, available=case["available"], order=case["order"],
                       done_rule="next" if bool(case["done_on_next"]) else "source", log=log)
    return res, gen


def planned(z):
    return [n for n in names(z) if not str(golden_case(z, n)["error"])]


def test_restatement_equals_reference_goldens(z):
    checked = 0
    for name in names(z):
        case = golden_case(z, name)
        if str(case["error"]) == "ZeroDivisionError":
            with pytest.raises(ZeroDivisionError):
                case_thresholds(case)
            continue
        res, gen = restate(case)
        assert res["env_steps"] == int(case["env_steps"]), name
        assert np.array_equal(native.rng_state_from_generator(gen), case["rng_after"]), name
        if str(case["error"]):
            assert str(case["error"]) == "ValueError" and res["error"] == {"reward_range": "range", "one_action": "one_action"}[name]
            continue
        assert res["error"] is None and np.array_equal(res["plan"], case["plan"]), name
        assert res["episodes_run"] == int(case["episodes_run"]), name
        tree = gr.as_bfs(res)
        for k in ("parent", "kind", "action", "depth", "count", "done", "cum", "mu_ucb", "mu_lcb", "vu", "vl"):
            assert np.array_equal(tree[k], case["tree/" + k]), (name, k)       # this host's numpy log, as the reference: bits
        checked += 1
    assert checked >= 13


@pytest.mark.parametrize("seed", [1, 2])
def test_no_golden_case_hangs_on_the_last_bits_of_log(z, seed):
    """The restatement with every ``log`` moved by up to 2 ulp gives the same plans, counts, episodes and generator records on
    EVERY golden case, those that raise included: the steps and draws before a raise hang on the same comparisons."""
    for name in names(z):
        case = golden_case(z, name)
        if str(case["error"]) == "ZeroDivisionError":
            with pytest.raises(ZeroDivisionError):       # (the threshold's eval raises before any log is taken)
                case_thresholds(case)
            continue
        res, gen = restate(case, log=gr.jittered_log(seed))
        assert np.array_equal(native.rng_state_from_generator(gen), case["rng_after"]), name
        assert res["env_steps"] == int(case["env_steps"]), name
        if str(case["error"]):
            assert res["error"] == {"reward_range": "range", "one_action": "one_action"}[name]
            continue
        assert np.array_equal(res["plan"], case["plan"]) and res["episodes_run"] == int(case["episodes_run"]), name
        tree = gr.as_bfs(res)
        for k in ("parent", "kind", "action", "depth", "count", "done", "cum"):
            assert np.array_equal(tree[k], case["tree/" + k]), (name, k)
        for k in ("mu_ucb", "mu_lcb", "vu", "vl"):
            assert np.all(np.abs(tree[k] - case["tree/" + k]) <= 1e-12 / (1 - float(case["gamma"]))), (name, k)


def test_goldens_cover_the_issue_cases(z):
    cases = {n: golden_case(z, n) for n in names(z)}
    ok = {n: c for n, c in cases.items() if not str(c["error"])}
    assert float(z["gape/margin"]) > 1e-9 and all(float(c["margin"]) > 1e-9 for c in ok.values())
    assert {str(c["continuation"]) for c in ok.values()} == {"zeros", "uniform"}
    masked = [c for c in ok.values() if not c["available"].all()]
    assert {str(c["continuation"]) for c in masked} == {"zeros", "uniform"} and all(int(c["unlisted"]) > 0 for c in masked)
    assert any(not np.array_equal(c["order"], np.arange(len(c["order"]))) for c in ok.values())
    assert any(bool(c["done_on_next"]) and c["tree/done"].any() for c in ok.values())
    assert any(bool(c["horizon_given"]) for c in ok.values()) and any(bool(c["horizon_from_accuracy"]) for c in ok.values())
    assert int(ok["early_stop"]["episodes_run"]) < int(ok["early_stop"]["episodes"])
    assert int(ok["full_run"]["episodes_run"]) == int(ok["full_run"]["episodes"]) + 2
    assert ok["wide_70"]["mdp/reward"].shape[1] == 70 and int(ok["wide_70"]["horizon"]) == 3
    assert 2 * int(ok["horizon_40"]["horizon"]) > 64
    assert all(int(c["tie_draws"]) > 0 for c in ok.values())
    assert str(cases["reward_range"]["error"]) == "ValueError" and int(cases["reward_range"]["env_steps"]) > 1
    assert str(cases["one_action"]["error"]) == "ValueError" and int(cases["one_action"]["env_steps"]) == 0
    assert str(cases["confidence_one"]["error"]) == "ZeroDivisionError" and int(cases["confidence_one"]["env_steps"]) == 1
    # plan-level cases hold no exact 0 / 1 rewards: those compare mathematically equal bounds reached by different arithmetic
    assert not any(((c["mdp/reward"] == 0) | (c["mdp/reward"] == 1)).any() for c in ok.values())


def test_lower_bound_restatement_equals_the_reference():
    g = np.load(os.path.join(HERE, "golden", "kl_lower_bound.npz"))
    for s, c, t, b, i, m in zip(g["total"], g["count"], g["threshold"], g["bound"], g["iterations"], g["decisions"]):
        assert gr.kl_bound_traced(float(s), int(c), float(t), lower=True) == (b, i, m), (s, c, t)
    assert {0, 1, 2, 4} <= set(g["decisions"].tolist()) and (g["bound"] == 0).any() and (g["total"] == g["count"]).any()


def env3():
    return FiniteMDPEnv(dict(generators.random_deterministic(10, 3, seed=1)))


def test_threshold_table_is_the_reference_eval():
    from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapE
    planner = MDPGapE(env3(), dict(budget=100, gamma=0.8))
    cfg = planner.config
    horizon, actions, confidence, time = cfg["horizon"], 3, cfg["confidence"], cfg["episodes"]  # noqa: F841
    table = planner.thresholds()
    assert len(table) == cfg["episodes"] + 2
    for count in range(1, len(table) + 1):
        assert table[count - 1] == eval(cfg["upper_bound"]["threshold"])
    assert np.array_equal(table, gr.thresholds_by_count(gr.DEFAULT_THRESHOLD, horizon, actions, confidence, time))
    assert cfg["upper_bound"]["threshold"] == gr.DEFAULT_THRESHOLD
    log_time = MDPGapE(env3(), dict(budget=100, gamma=0.8, upper_bound=dict(threshold="1*np.log(time)")))
    assert np.array_equal(log_time.thresholds(), np.full(log_time.config["episodes"] + 2, 1 * np.log(log_time.config["episodes"])))
    with pytest.raises(ZeroDivisionError):
        MDPGapE(env3(), dict(budget=100, confidence=1.0)).thresholds()


def test_budget_split_and_initial_values():
    from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapE
    from rl_agents_amd.agents.tree_search.olop import OLOP
    planner = MDPGapE(env3(), dict(budget=300, gamma=0.8))
    assert (planner.config["episodes"], planner.config["horizon"]) == OLOP.allocation(300, 0.8)
    acc = MDPGapE(env3(), dict(budget=300, gamma=0.8, accuracy=0.5, horizon_from_accuracy=True))
    h = int(np.ceil(np.log(0.5 * (1 - 0.8) / 2) / np.log(0.8)))
    assert (acc.config["horizon"], acc.config["episodes"]) == (h, 300 // h)
    with pytest.raises(AssertionError):
        MDPGapE(env3(), dict(budget=h, gamma=0.8, accuracy=0.5, horizon_from_accuracy=True))
    assert MDPGapE.value_init(0.8, 5).tolist() == [(1 - 0.8 ** (5 - d)) / (1 - 0.8) for d in range(6)]
    assert planner.config["accuracy"] == 1.0 and planner.config["confidence"] == 0.9 and planner.budget_used == 0
    assert planner.config["continuation_type"] == "uniform" and planner.config["max_next_states_count"] == 1


class NoDevice(object):
    """Stands where the model cache is: a refusal must come before anything is uploaded."""

    def __getattr__(self, name):
        raise AssertionError("the device was asked for " + name)


def test_refusals():
    with pytest.raises(NotImplementedError, match="subtree"):
        agent_factory(env3(), {"__class__": GAPE_AGENT, "step_strategy": "subtree"})
    agent = agent_factory(env3(), {"__class__": GAPE_AGENT, "budget": 50, "max_next_states_count": 2})
    agent.planner.models = NoDevice()
    with pytest.raises(NotImplementedError, match="placeholder"):
        agent.planner.plan_batch(env3(), [0])
    agent = agent_factory(env3(), {"__class__": GAPE_AGENT, "budget": 50, "upper_bound": {"type": "hoeffding"}})
    agent.planner.models = NoDevice()
    with pytest.raises(ValueError, match="only logs"):
        agent.planner.plan_batch(env3(), [0])
    for stoch in (generators.random_stochastic(10, 3, seed=2), generators.random_sparse(10, 3, 2, seed=3)):
        env = FiniteMDPEnv(dict(stoch))
        agent = agent_factory(env, {"__class__": GAPE_AGENT, "budget": 50})
        with pytest.raises(TypeError, match="deterministic"):
            agent.planner.plan_batch(env, [0])
    with pytest.raises(TypeError):
        agent_factory(env3(), {"__class__": GAPE_AGENT, "upper_bound": "kullback-leibler"})
    with pytest.raises(ZeroDivisionError):
        agent_factory(env3(), {"__class__": GAPE_AGENT, "gamma": 1.0, "horizon": 3, "episodes": 4})


def test_per_episode_evaluation_refuses_the_agent():
    from rl_agents_amd.agents.tree_search.olop import OLOP
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    agent = agent_factory(env3(), {"__class__": GAPE_AGENT, "budget": 50})
    assert isinstance(agent.planner, OLOP) and agent.planner.supports_device_loop() is False
    with pytest.raises(NotImplementedError, match="one model per episode"):
        PerEpisodeEvaluation([env3(), env3()], agent)


@pytest.mark.parametrize("name", sorted(REFERENCE_CONFIGS))
def test_reference_configs_load_with_the_class_line_changed(name):
    from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapE, MDPGapEAgent
    assert REFERENCE_CONFIGS[name]["__class__"] == "<class 'rl_agents.agents.tree_search.mdp_gape.MDPGapEAgent'>"
    cfg = dict(REFERENCE_CONFIGS[name], __class__=GAPE_AGENT)
    cfg.pop("env_preprocessors", None)          # (highway-env's "simplify": the finite-MDP env has no such method)
    agent = agent_factory(env3(), cfg)
    assert isinstance(agent, MDPGapEAgent) and isinstance(agent.planner, MDPGapE)
    pc = agent.planner.config
    assert pc["upper_bound"]["threshold"] == "1*np.log(time)" and pc["upper_bound"]["transition_threshold"] == "0.1*np.log(time)"
    assert pc["episodes"] * pc["horizon"] <= max(pc["budget"], 3) and pc["accuracy"] == cfg["accuracy"]


def test_agent_steps_as_the_reference():
    agent = agent_factory(env3(), {"__class__": GAPE_AGENT, "budget": 50, "receding_horizon": 3})
    assert agent.step([]) is True and agent.remaining_horizon == 2
    assert agent.step([1]) is True and agent.remaining_horizon == 1           # the reset tree has no children: replan
    agent.record(0, 1, 0.5, 7, False, {})
    assert agent.planner.next_observation == 7


def test_header_signatures_and_library_have_the_entry_points():
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    assert re.search(r"\bint mp_gape_plan\(mp_ctx \*ctx, mp_model \*model, int32_t n_roots", header)
    assert re.search(r"\bint mp_gape_tree_export\(mp_ctx \*ctx, int32_t root, int32_t cap, int32_t \*n_nodes, uint8_t \*kind", header)
    assert re.search(r"\bconst char \*mp_gape_form_names\(void\);", header)
    assert re.search(r"#define\s+MP_ERR_GAPE_NO_CHALLENGER\s+\(-9\)", header)
    assert re.search(r"#define\s+MP_ABI_VERSION\s+7\b", header)
    lib = native.load()
    assert lib.mp_abi_version() == 7
    for symbol in ("mp_gape_plan", "mp_gape_tree_export", "mp_gape_form_names"):
        assert symbol in native.SIGNATURES and getattr(lib, symbol) is not None, symbol
    # one pointer or number per declared parameter
    for symbol in ("mp_gape_plan", "mp_gape_tree_export"):
        declared = re.search(r"\bint %s\(([^;]*)\);" % symbol, header).group(1)
        assert len(native.SIGNATURES[symbol][1]) == declared.count(",") + 1, symbol
    form_names = native.gape_form_names()
    assert form_names == ["gape_global", "gape_global_slots"]
    for other in (native.kernel_form_names(), native.each_form_names(), native.ss_form_names(), native.olop_stoch_form_names()):
        assert not set(form_names) & set(other)
    assert native.ERR_GAPE_NO_CHALLENGER == -9


# ---- the sweep of tests/test_gpu_gape_sweep.py: what it holds, on the restatement alone -----------------------------------------
@pytest.fixture(scope="module")
def sweep():
    """[(case, [(result, generator record after, observations) per root])] of every case."""
    cases = [gc.sweep_case(i) for i in range(gc.N_CASES)]
    return [(case, gc.restate_case(case)) for case in cases]


def seen_of(plan, kind):
    return [v for k, v in plan[2] if k == kind]


def test_sweep_skips_at_most_the_cap(sweep):
    """A cap, not a measurement: 7 of 202 plans (3.5 %) have a margin <= 1e-9 -- values that are equal on paper and reached by
    different arithmetic on the three-valued reward grids, 2e-16 .. 1e-15 apart."""
    plans = [p for _, restated in sweep for p in restated]
    close = sum(1 for p in plans if p[0]["error"] is None and gc.margin(p[2]) <= gc.MARGIN)
    print("sweep: {} plans, {} with margin <= {}".format(len(plans), close, gc.MARGIN))
    assert len(plans) == gc.N_CASES * gc.ROOTS == 202
    assert close <= gc.SKIP_CAP * len(plans), close


def test_sweep_cases_are_drawn_as_the_docstring_says():
    for i in range(gc.N_RANDOM):
        case = gc.sweep_case(i)
        n_states, n_actions = case["mdp/reward"].shape
        wide, reward = i % 6 == 5, case["mdp/reward"]
        assert 2 <= n_states < 40 and (65 <= n_actions < 151 if wide else 2 <= n_actions < 10), i
        assert reward.min() >= 1e-3 and reward.max() <= 1 - 1e-3, i
        assert case["available"].all() or i % 3 == 1, i
        assert np.array_equal(case["order"], np.arange(n_actions)) or i % 6 == 1, i
        assert int(case["horizon"]) in (gc.WIDE_HORIZONS if wide else gc.HORIZONS), i
        assert 1 <= int(case["episodes"]) < (6 if int(case["horizon"]) >= 32 else 25), i
        assert len(case["roots"]) == gc.ROOTS and len({r.tobytes() for r in case["rng"]}) == gc.ROOTS, i
        again = gc.sweep_case(i)
        assert all(np.array_equal(case[k], again[k]) for k in case), i
    rounded = sum(1 for i in range(gc.N_RANDOM) if set(np.unique(gc.sweep_case(i)["mdp/reward"])) <= {0.25, 0.5, 0.75})
    assert gc.N_RANDOM // 6 <= rounded <= gc.N_RANDOM // 2, rounded


def test_sweep_contains_the_cases_it_is_for(sweep):
    def some(pred):
        return any(pred(case, plan) for case, restated in sweep for plan in restated)

    def width(case):
        return case["mdp/reward"].shape[1]

    def masked(case):
        return not case["available"].all()

    def uniform(case):
        return str(case["continuation"]) == "uniform"
    # a mask over more than 64 actions, uniform continuation: an unlisted action drawn (rank 0), and a listed one whose column
    # lies in the second and in the third chunk with unlisted actions before it
    assert some(lambda c, p: masked(c) and width(c) > 64 and uniform(c) and any(v[1] == 0 for v in seen_of(p, "continuation")))
    for first in (64, 128):
        assert some(lambda c, p: masked(c) and width(c) > 64 and uniform(c)
                    and any(v[1] == 1 and v[2] >= first for v in seen_of(p, "continuation"))), first
    assert some(lambda c, p: width(c) > 128)
    # a tie set of more than 64 members, the drawn one past its 64th and past its 128th (the rank carried over one and two chunks)
    for rank in (63, 127):
        assert some(lambda c, p: any(v[0] > 64 and v[1] > rank for v in seen_of(p, "ties"))), rank
    for horizon in (32, 33, 70):
        assert some(lambda c, p: int(c["horizon"]) == horizon and p[0]["error"] is None), horizon
    for continuation in ("uniform", "zeros"):
        assert some(lambda c, p: masked(c) and str(c["continuation"]) == continuation and p[0]["error"] is None), continuation
    for on_next in (False, True):
        assert some(lambda c, p: bool(c["done_on_next"]) == on_next and p[0]["done"].any()), on_next
    assert some(lambda c, p: p[0]["error"] is None and p[0]["episodes_run"] < int(c["episodes"]) + 2)
    assert some(lambda c, p: p[0]["error"] is None and p[0]["episodes_run"] == int(c["episodes"]) + 2)
    assert some(lambda c, p: p[0]["error"] == "one_action" and p[0]["env_steps"] == 0)
    assert some(lambda c, p: not np.array_equal(c["order"], np.arange(width(c))) and p[0]["error"] is None)
    assert {str(c["threshold"]) for c, _ in sweep} == {gr.DEFAULT_THRESHOLD, gc.LOG_TIME}
    assert not any(p[0]["error"] == "range" for _, restated in sweep for p in restated)


def test_restatement_reports_its_draws(z):
    """The observations the contents above are read from, on a golden case whose numbers the golden file holds."""
    case = golden_case(z, "masked_uniform")
    res, _, seen = gc.restate_plan(dict(case), int(case["s0"]), case["rng_before"], case_thresholds(case))
    assert np.array_equal(res["plan"], case["plan"])
    cont = [v for k, v in seen if k == "continuation"]
    ties = [v for k, v in seen if k == "ties"]
    assert sum(1 for v in cont if v[1] == 0) == int(case["unlisted"]) > 0
    assert sum(1 for v in ties if v[0] > 1) == int(case["tie_draws"]) > 0
    assert all(0 <= v[1] < v[0] for v in ties) and all(v[2] == v[0] for v in cont)          # (identity order: column = action)
    assert gc.margin(seen) == pytest.approx(float(case["margin"])) or gc.margin(seen) < float(case["margin"])
    assert gc.margin(seen) > gc.MARGIN


def test_margins_of_the_batch_tests_of_the_device():
    """The roots that test_300_roots_against_the_restatement and test_more_trees_than_the_workspace_keeps (tests/test_gpu_gape.py)
    compare with the restatement: no comparison of theirs is closer than 1e-9."""
    from tests.test_gpu_gape import SMALL_CFG, small_case, small_env
    env = small_env()
    for seed, n, sample in ((11, 300, range(300)), (13, 40000, (0, 1, 255, 256, 8192, 8193, 20001, 39999))):
        agent = agent_factory(env, dict(SMALL_CFG, __class__=GAPE_AGENT))
        agent.seed(seed)
        rng = agent.planner.batch_rng_states(n)
        thr = None
        for i in sample:
            case = small_case(i % 12, rng[i])
            thr = case_thresholds(case) if thr is None else thr
            res, _, seen = gc.restate_plan(case, i % 12, rng[i], thr)
            assert res["error"] is None and gc.margin(seen) > gc.MARGIN, (seed, i, gc.margin(seen))
