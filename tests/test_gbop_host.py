"""GBOP on the host: the test-side restatement against the reference's own outputs (tests/golden/gbop.npz), the C ABI's
declarations, the config, the factory name, the reference's exceptions from the status codes and the threshold tables by
lifetime count -- no GPU needed."""
import json
import os
import re

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv, generators
from tests import gbop_restatement as gb

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gbop.npz")
GBOP_AGENT = "<class 'rl_agents_amd.agents.tree_search.graph_based_stochastic.StochasticGraphBasedPlannerAgent'>"
ENTRY_POINTS = {"mp_gbop_create": 6, "mp_gbop_free": 1, "mp_gbop_plan": 23, "mp_gbop_info": 8, "mp_gbop_export": 26,
                "mp_gbop_form_names": 0}
BOUND_TOL = 1e-12                     # times 1 / (1 - gamma): the project's tolerance for this solve
ERRORS = ("placeholders", "default_config", "no_listed_action")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def golden_case(z, name):
    p = "gbop/" + name
    return {k[len(p) + 1:]: z[k] for k in z.files if k.startswith(p + "/")}


def names(z):
    return [str(n) for n in z["gbop/names"]]


def generator_from(state6):
    gen = np.random.Generator(np.random.PCG64(0))
    native.generator_set_state(gen, state6)
    return gen


def golden_graph(case, i):
    p = "plan{}/graph/".format(i)
    return gb.unpack_listing({k[len(p):]: v for k, v in case.items() if k.startswith(p)})


def graph_of(case):
    return gb.Graph(str(case["mdp/mode"]), case["mdp/transition"], case["mdp/reward"], float(case["gamma"]),
                    int(case["max_next_states_count"]), case.get("mdp/next"), case["available"] if bool(case["masked"]) else None,
                    case["order"] if bool(case["ordered"]) else None)


def thresholds_of(case):
    A = case["mdp/reward"].shape[1]
    args = (int(case["horizon"]), A, int(case["episodes"]))
    return (lambda c: gb.thresholds_by_count(str(case["threshold"]), *args, c, c)[0],
            lambda c: gb.thresholds_by_count(str(case["transition_threshold"]), *args, c, c)[0])


def case_env(case, s0=0):
    c = dict(mode=str(case["mdp/mode"]), transition=case["mdp/transition"].tolist(), reward=case["mdp/reward"].tolist(),
             terminal=case["mdp/terminal"].astype(int).tolist(), state=int(s0), max_steps=0)
    if c["mode"] == "sparse":
        c["next"] = case["mdp/next"].tolist()
    if bool(case["ordered"]):
        env = OrderedMaskedFiniteMDPEnv(dict(c, available=case["available"].astype(int).tolist(),
                                             listing_order=[int(a) for a in case["order"]]))
    elif bool(case["masked"]):
        env = MaskedFiniteMDPEnv(dict(c, available=case["available"].astype(int).tolist()))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def case_config(case):
    cfg = {"__class__": GBOP_AGENT, "budget": int(case["budget"]), "gamma": float(case["gamma"]), "accuracy": float(case["accuracy"]),
           "sampling_timeout": int(case["sampling_timeout"]), "max_next_states_count": int(case["max_next_states_count"]),
           "upper_bound": {"type": "kullback-leibler", "threshold": str(case["threshold"]),
                           "transition_threshold": str(case["transition_threshold"])}}
    if bool(case["horizon_given"]):
        cfg.update(horizon=int(case["horizon"]), episodes=int(case["episodes"]))
    return cfg


def replay(case, i, graph):
    """Plan i of a golden case on the restatement -> (plan, exception or None, generator after)."""
    gen = generator_from(case["plan{}/rng_before".format(i)])
    rthr, tthr = thresholds_of(case)
    try:
        plan = graph.plan(int(case["roots"][i]), int(case["episodes"]), int(case["horizon"]), float(case["accuracy"]), rthr, tthr,
                          gen, int(case["sampling_timeout"]))
        return plan, None, gen
    except (ValueError, TypeError) as e:
        return [], e, gen


def golden_plan(case, i):
    p = "plan{}/".format(i)
    n = int(case[p + "plan_len"])
    plan = [int(case[p + "action"])] if n >= 1 else []
    if n >= 2:
        key = int(case[p + "key"])
        plan.append("placeholder_{}".format(-1 - key) if key < 0 else str(key))
    return plan


def test_restatement_equals_reference_goldens(z):
    plans = 0
    for name in names(z):
        case = golden_case(z, name)
        graph = graph_of(case)
        tol = BOUND_TOL / (1 - float(case["gamma"]))
        for i in range(int(case["n_plans"])):
            plan, error, gen = replay(case, i, graph)
            tag = (name, i)
            assert np.array_equal(native.rng_state_from_generator(gen), case["plan{}/rng_after".format(i)]), tag
            assert plan == golden_plan(case, i), tag
            assert ("" if error is None else type(error).__name__) == str(case["plan{}/error".format(i)]), tag
            if error is not None:
                assert str(error) == str(case["plan{}/message".format(i)]), tag
            assert graph.n_observations == int(case["plan{}/env_steps".format(i)]), tag
            assert gb.compare_listing(graph.listing(), golden_graph(case, i), tol) == [], tag
            plans += 1
    assert plans == sum(int(z["gbop/{}/n_plans".format(n)]) for n in names(z)) >= 18


def test_goldens_cover_the_issue_cases(z):
    cases = {n: golden_case(z, n) for n in names(z)}
    assert set(ERRORS) <= set(cases)
    assert {str(c["mdp/mode"]) for c in cases.values()} == {"deterministic", "stochastic", "sparse"}
    assert {int(c["max_next_states_count"]) for c in cases.values()} >= {1, 2, 3}
    assert any(bool(c["ordered"]) and not c["available"].all() for c in cases.values())
    assert sum(int(c["n_plans"]) == 3 and not str(c["plan2/error"]) for c in cases.values()) >= 2   # kept graph and counts
    last = lambda c: "plan{}/".format(int(c["n_plans"]) - 1)  # noqa: E731
    c = cases["placeholders"]
    assert str(c[last(c) + "error"]) == "ValueError" and str(c[last(c) + "message"]) == gb.NO_PLACEHOLDER
    c = cases["default_config"]
    assert str(c["plan0/error"]) == "TypeError" and str(c["plan0/message"]) == gb.REWARD_THRESHOLD
    assert str(c["threshold"]) == "1*np.log(time)" and int(c["plan0/env_steps"]) == 1
    assert not np.array_equal(c["plan0/rng_before"], c["plan0/rng_after"])       # the seed draw was made before the raise
    c = cases["no_listed_action"]
    assert str(c[last(c) + "error"]) == "ValueError" and not c["available"].any(axis=1).all()
    assert float(z["gbop/margin"]) > 1e-9                                        # asserted when the file was made
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "gape_stoch.npz"))
    # the reference's own configs: SailingEnv/agents/gbop.json and the "GBOP" entry of planners_evaluation.py
    assert (int(cases["sparse_b3_sailing"]["max_next_states_count"]), float(cases["sparse_b3_sailing"]["gamma"])) == (3, 0.9)
    assert float(cases["dense_b3_evaluation"]["accuracy"]) == 5e-2


def test_header_and_signatures_declare_the_entry_points():
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    for symbol, n_args in ENTRY_POINTS.items():
        assert re.search(r"\b%s\(" % symbol, header), symbol
        assert symbol in native.SIGNATURES, symbol
        assert len(native.SIGNATURES[symbol][1]) == n_args, symbol
    assert re.search(r"typedef struct mp_gbop mp_gbop;", header)
    assert re.search(r"#define MP_ABI_VERSION 7\b", header)
    for code, value in (("MP_ERR_GBOP_PLACEHOLDERS", native.ERR_GBOP_PLACEHOLDERS),
                        ("MP_ERR_GBOP_REWARD_THRESHOLD", native.ERR_GBOP_REWARD_THRESHOLD),
                        ("MP_ERR_GBOP_CHOICE_P", native.ERR_GBOP_CHOICE_P)):
        assert re.search(r"#define %s \(%d\)" % (code, value), header), code


def test_library_exports_the_symbols_and_its_own_form_names():
    lib = native.load()
    for symbol in ENTRY_POINTS:
        assert getattr(lib, symbol) is not None, symbol
    forms = native.gbop_form_names()
    assert sorted(forms) == sorted("gbop_{}_{}".format(m, p) for m in ("table", "dense", "sparse") for p in ("lds", "global"))
    others = (native.kernel_form_names() + native.each_form_names() + native.gape_form_names() + native.gape_stoch_form_names()
              + native.olop_stoch_form_names() + native.ss_form_names())
    assert not set(forms) & set(others)


def test_default_config_and_factory():
    from rl_agents_amd import gbop
    from rl_agents_amd.agents.tree_search import graph_based_stochastic as module
    env = FiniteMDPEnv(dict(generators.random_sparse(10, 3, 2, seed=1)))
    agent = agent_factory(env, {"__class__": GBOP_AGENT})
    assert type(agent) is module.StochasticGraphBasedPlannerAgent is gbop.StochasticGraphBasedPlannerAgent
    assert type(agent.planner) is module.StochasticGraphBasedPlanner and agent.PLANNER_TYPE is module.StochasticGraphBasedPlanner
    assert module.StochasticGraphBasedPlanner.NODE_TYPE is module.GraphDecisionNode
    pc = agent.planner.config
    assert (pc["budget"], pc["gamma"], pc["step_strategy"]) == (500, 0.8, "reset")
    assert (pc["sampling_timeout"], pc["accuracy"], pc["max_next_states_count"]) == (100, 1e-2, 1)
    assert pc["upper_bound"] == {"type": "kullback-leibler", "time": "global", "threshold": "1*np.log(time)",
                                 "transition_threshold": "0.1*np.log(time)"}
    assert (pc["episodes"], pc["horizon"]) == native.olop_allocation(500, 0.8)
    planner = agent.planner
    assert planner.carries_state is True and planner.supports_per_episode_tables is False and planner.per_episode_kind is None
    assert planner.supports_device_loop() is False and planner.plan_batch_device is None
    assert planner.nodes == {} and planner.root is None and dict(planner.get_visits()) == {} and dict(planner.get_updates()) == {}
    assert planner.get_plan() == []
    # a budget below the action count is raised to it (:342); "horizon" in the config keeps the config's split
    small = agent_factory(env, {"__class__": GBOP_AGENT, "budget": 1}).planner.config
    assert (small["episodes"], small["horizon"]) == native.olop_allocation(3, 0.8)
    given = agent_factory(env, {"__class__": GBOP_AGENT, "horizon": 4, "episodes": 7}).planner.config
    assert (given["episodes"], given["horizon"]) == (7, 4)
    with pytest.raises(ZeroDivisionError):
        agent_factory(env, {"__class__": GBOP_AGENT, "gamma": 1})


def test_the_reference_config_loads_with_only_its_prefix_changed():
    with open(os.path.join(HERE, "golden", "gbop_sailing_config.json")) as f:
        cfg = json.load(f)
    assert cfg["__class__"] == "<class 'rl_agents.agents.tree_search.graph_based_stochastic.StochasticGraphBasedPlannerAgent'>"
    cfg["__class__"] = cfg["__class__"].replace("'rl_agents.", "'rl_agents_amd.")
    assert cfg["__class__"] == GBOP_AGENT
    env = FiniteMDPEnv(dict(generators.random_stochastic(6, 3, seed=2)))
    planner = agent_factory(env, cfg).planner
    assert (planner.config["max_next_states_count"], planner.config["gamma"], planner.config["budget"]) == (3, 0.9, 1000)
    assert planner.config["upper_bound"]["threshold"] == "0*np.log(time)"


def test_status_codes_raise_the_reference_exceptions():
    from rl_agents_amd.gbop import PLACEHOLDERS_MESSAGE, REWARD_THRESHOLD_MESSAGE, StochasticGraphBasedPlanner as P
    assert PLACEHOLDERS_MESSAGE == gb.NO_PLACEHOLDER and REWARD_THRESHOLD_MESSAGE == gb.REWARD_THRESHOLD
    ok = np.zeros(3, np.int32)
    P.raise_for_status(ok)

    def one(code):
        status = ok.copy()
        status[1] = code
        return status
    with pytest.raises(ValueError) as e:
        P.raise_for_status(one(native.ERR_GBOP_PLACEHOLDERS))
    assert str(e.value) == PLACEHOLDERS_MESSAGE
    with pytest.raises(TypeError) as e:
        P.raise_for_status(one(native.ERR_GBOP_REWARD_THRESHOLD))
    assert str(e.value) == REWARD_THRESHOLD_MESSAGE
    with pytest.raises(ValueError, match="probabilities do not sum to 1"):
        P.raise_for_status(one(native.ERR_GBOP_CHOICE_P))
    with pytest.raises(ValueError, match="zero-size array to reduction operation maximum"):
        P.raise_for_status(one(native.MP_ERR_GBOPD_NO_ACTION))
    with pytest.raises(RuntimeError, match="2\\*\\*22 queue pops"):
        P.raise_for_status(one(native.MP_ERR_GBOPD_DIVERGED))
    with pytest.raises(RuntimeError, match="queue overflow"):
        P.raise_for_status(one(native.MP_ERR_ALLOC))
    with pytest.raises(RuntimeError, match="root state is out of range"):
        P.raise_for_status(one(native.MP_ERR_ARG))


def test_threshold_tables_grow_by_the_new_counts_only():
    """Lifetime counts across three plans give the same tables as evaluating from scratch, and no count is evaluated twice."""
    from rl_agents_amd.gbop import ThresholdTables
    bound = {"threshold": "0*np.log(time)", "transition_threshold": "0.1*np.log(time) + 0.05*np.log(1 + count)"}
    tables, reach = ThresholdTables(), 0
    for _ in range(3):
        reach += 12 * 7
        reward, transition = tables.upto(bound, 7, 3, 12, reach)
        assert reward.size == transition.size == reach and tables.evaluations == reach
        assert np.array_equal(reward, gb.thresholds_by_count(bound["threshold"], 7, 3, 12, 1, reach))
        assert np.array_equal(transition, gb.thresholds_by_count(bound["transition_threshold"], 7, 3, 12, 1, reach))
    tables.upto(bound, 7, 3, 12, 10)
    assert tables.evaluations == reach                                   # nothing new to evaluate
    tables.upto(dict(bound, threshold="1*np.log(time)"), 7, 3, 12, 5)    # another string: another table
    assert tables.reward.size == 5 and np.all(tables.reward == np.log(12))


def test_exported_nodes_from_a_listing(z):
    """build_graph: decision nodes by str(observation) in creation order, chance nodes by action in listing order, transition
    children keyed and ordered as the reference's dict, parents as ordered lists."""
    from rl_agents_amd.gbop import GraphChanceNode, GraphDecisionNode, build_graph
    case = golden_case(z, "sparse_b2_k3")
    lst = golden_graph(case, 0)
    nodes = build_graph(lst)
    assert list(nodes) == [str(s) for s in lst["state"]]
    seen_placeholder = seen_state = False
    for i, node in enumerate(nodes.values()):
        assert isinstance(node, GraphDecisionNode) and node.observation == int(lst["state"][i]) and node.count == int(lst["count"][i])
        assert (node.value_lower, node.value_upper) == (lst["lower"][i], lst["upper"][i])
        k = int(lst["n_children"][i])
        assert list(node.children) == lst["action"][i, :k].tolist()
        assert [p.observation for p in node.parents] == \
            lst["state"][lst["parent_idx"][lst["parent_ptr"][i]:lst["parent_ptr"][i + 1]]].tolist()
        for j, ch in enumerate(node.children.values()):
            assert isinstance(ch, GraphChanceNode) and ch.parent is node and ch.count == int(lst["c_count"][i, j])
            assert (ch.value_lower, ch.value_upper) == (lst["c_lower"][i, j], lst["c_upper"][i, j])
            keys = ["placeholder_{}".format(-1 - s) if s < 0 else str(s) for s in lst["k_state"][i, j]]
            assert list(ch.children) == keys
            assert [d.count for d in ch.children.values()] == lst["k_count"][i, j].tolist()
            assert [d.cumulative_reward for d in ch.children.values()] == lst["k_cum"][i, j].tolist()
            assert [d.mu_ucb for d in ch.children.values()] == lst["k_mu_ucb"][i, j].tolist()
            assert [d.mu_lcb for d in ch.children.values()] == lst["k_mu_lcb"][i, j].tolist()
            seen_placeholder |= any(s < 0 for s in lst["k_state"][i, j])
            seen_state |= any(s >= 0 for s in lst["k_state"][i, j])
            if ch.count:
                assert np.array_equal(ch.p_hat, lst["k_count"][i, j] / ch.count)
            if lst["c_backed"][i, j] >= 0:
                assert np.array_equal(ch.p_plus, lst["p_plus"][i, j]) and np.array_equal(ch.p_minus, lst["p_minus"][i, j])
                assert len(ch.next_states) == len(keys) and sorted(ch.next_states) == sorted(keys)
            else:
                assert ch.p_plus is None and ch.p_minus is None and ch.next_states is None
    assert seen_placeholder and seen_state


def test_per_episode_tables_are_refused_with_the_reason():
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    envs = [FiniteMDPEnv(dict(generators.random_deterministic(10, 3, seed=s))) for s in (1, 2)]
    agent = agent_factory(envs[0], {"__class__": GBOP_AGENT})
    with pytest.raises(NotImplementedError, match="StochasticGraphBasedPlanner keeps its planner state"):
        PerEpisodeEvaluation(envs, agent)


def test_planners_for_stochastic_envs_take_the_environment_generator_records():
    """BatchedEvaluation hands ``env_rng_states`` to ``plan_batch`` on stochastic envs: the planners that re-seed their clones
    accept it."""
    import inspect
    from rl_agents_amd.agents.tree_search.brue import BRUE
    from rl_agents_amd.agents.tree_search.olop import StochasticOLOP
    from rl_agents_amd.gape_stochastic import StochasticMDPGapE
    from rl_agents_amd.gbop import StochasticGraphBasedPlanner
    for cls in (BRUE, StochasticOLOP, StochasticMDPGapE, StochasticGraphBasedPlanner):
        assert inspect.signature(cls.plan_batch).parameters["env_rng_states"].default is None, cls.__name__
