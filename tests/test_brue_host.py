"""BRUE on the host: the test-side restatement against the reference's own outputs (tests/golden/brue.npz), the C ABI's
declarations, the budget split, the config and the refusals of BRUEAgent -- no GPU needed."""
import os
import re

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, generators
from tests import brue_restatement as br

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "brue.npz")
BRUE_AGENT = "<class 'rl_agents_amd.agents.tree_search.brue.BRUEAgent'>"


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def golden_case(z, name):
    p = "brue/" + name
    return {k[len(p) + 1:]: z[k] for k in z.files if k.startswith(p + "/")}


def names(z):
    return [str(n) for n in z["brue/names"]]


def generator_from(state6):
    gen = np.random.Generator(np.random.PCG64(0))
    native.generator_set_state(gen, state6)
    return gen


def restate(case):
    """Run the restatement on one golden case's inputs; returns (result, generator after)."""
    gen = generator_from(case["rng_before"])
    res = br.brue_plan(str(case["mdp/mode"]), case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"],
                       int(case["s0"]), int(case["budget"]), int(case["horizon"]), float(case["gamma"]), gen,
                       nxt=case.get("mdp/next"), done_rule="next" if bool(case["done_on_next"]) else "source")
    return res, gen


def test_restatement_equals_reference_goldens(z):
    checked = 0
    for name in names(z):
        case = golden_case(z, name)
        res, gen = restate(case)
        assert res["env_steps"] == int(case["env_steps"]), name
        assert np.array_equal(native.rng_state_from_generator(gen), case["rng_after"]), name
        if str(case["error"]):
            assert str(case["error"]) == "ValueError" and res["error"] == "empty", name
            continue
        assert res["error"] is None, name
        assert np.array_equal(res["plan"], case["plan"]), name
        tree = br.as_bfs(res)
        for k in br.TREE_KEYS:              # f64 by bits: array_equal on finite values, and the sign of zero
            assert np.array_equal(tree[k], case["tree/" + k]), (name, k)
        assert np.array_equal(tree["stat"].view(np.uint64), case["tree/stat"].view(np.uint64)), name
        visits = br.visits_of(res)
        assert sorted(visits) == [str(k) for k in case["visit_keys"]], name
        assert [visits[str(k)] for k in case["visit_keys"]] == case["visit_counts"].tolist(), name
        checked += 1
    assert checked >= 20


def test_goldens_cover_the_issue_cases(z):
    cases = {n: golden_case(z, n) for n in names(z)}
    planned = {n: c for n, c in cases.items() if not str(c["error"])}
    assert {str(c["mdp/mode"]) for c in planned.values()} == {"deterministic", "stochastic", "sparse"}
    for rule in (False, True):              # terminal states under both done rules; a root that is terminal
        assert any(c["mdp/terminal"].any() and bool(c["done_on_next"]) == rule for c in planned.values())
    assert any(c["mdp/terminal"][int(c["s0"])] for c in planned.values())
    assert any(set(np.unique(c["mdp/reward"])) <= {0.0, 1.0} and restate(c)[0]["ties"] >= 2 for c in planned.values())
    assert any(c["mdp/reward"].shape[1] == 1 for c in planned.values())
    assert any(0 < int(c["budget"]) < c["mdp/reward"].shape[1] for c in planned.values())
    assert any(int(c["budget"]) == 0 and str(c["error"]) == "ValueError" for c in cases.values())
    assert any(bool(c["horizon_given"]) for c in planned.values())
    assert any(not c["available"].all() for c in planned.values())
    assert {float(c["gamma"]) for c in planned.values()} >= {0.7, 0.8, 0.95}
    assert max(int(c["budget"]) for c in planned.values()) >= 1000
    assert len(z["brue_episode/actions"]) == 8


def test_header_and_signatures_declare_the_entry_points():
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    for symbol in ("mp_brue_plan", "mp_brue_tree_export"):
        assert re.search(r"\bint %s\(mp_ctx \*ctx" % symbol, header), symbol
        assert symbol in native.SIGNATURES, symbol
    assert len(native.SIGNATURES["mp_brue_plan"][1]) == 14
    assert len(native.SIGNATURES["mp_brue_tree_export"][1]) == 10
    assert re.search(r"#define MP_ABI_VERSION 7\b", header)


def test_default_config_and_budget_split_equal_the_goldens(z):
    from rl_agents_amd.agents.tree_search.brue import BRUE
    from rl_agents_amd.agents.tree_search.olop import OLOP
    assert issubclass(BRUE, OLOP)
    for name in names(z):
        case = golden_case(z, name)
        cfg = dict(mode=str(case["mdp/mode"]), transition=case["mdp/transition"], reward=case["mdp/reward"],
                   terminal=case["mdp/terminal"])
        if "mdp/next" in case:
            cfg["next"] = case["mdp/next"]
        env = FiniteMDPEnv(cfg)
        agent_cfg = {"__class__": BRUE_AGENT, "budget": int(case["budget"]), "gamma": float(case["gamma"])}
        if bool(case["horizon_given"]):
            agent_cfg["horizon"] = int(case["horizon"])
        pc = agent_factory(env, agent_cfg).planner.config
        assert pc["horizon"] == int(case["horizon"]), name
        assert pc.get("episodes", -1) == int(case["episodes"]), name
        assert (pc["budget"], pc["gamma"], pc["step_strategy"]) == (int(case["budget"]), float(case["gamma"]),
                                                                    str(case["step_strategy"])), name
    env = FiniteMDPEnv(dict(generators.random_deterministic(10, 5, seed=1)))
    pc = agent_factory(env, {"__class__": BRUE_AGENT}).planner.config
    assert (pc["budget"], pc["gamma"], pc["step_strategy"]) == (500, 0.8, "reset")
    assert (pc["episodes"], pc["horizon"]) == OLOP.allocation(500, 0.8)
    pc = agent_factory(env, {"__class__": BRUE_AGENT, "budget": 2}).planner.config      # max(|A|, budget)
    assert (pc["episodes"], pc["horizon"]) == OLOP.allocation(5, 0.8)


def test_gamma_powers_are_python_arithmetic():
    from rl_agents_amd.agents.tree_search.brue import BRUE
    assert BRUE.gamma_powers(0.8, 9).tolist() == [0.8 ** d for d in range(10)]


def test_agent_factory_resolves_brue_agent_and_subtree_is_refused():
    from rl_agents_amd.agents.tree_search.brue import BRUE, BRUEAgent
    for tab in (generators.random_deterministic(10, 3, seed=1), generators.random_stochastic(10, 3, seed=2),
                generators.random_sparse(10, 3, 2, seed=3)):
        agent = agent_factory(FiniteMDPEnv(dict(tab)), {"__class__": BRUE_AGENT, "budget": 50})
        assert isinstance(agent, BRUEAgent) and isinstance(agent.planner, BRUE)
        assert agent.planner.supports_device_loop() is False
    with pytest.raises(NotImplementedError, match="subtree"):
        agent_factory(FiniteMDPEnv(dict(generators.random_deterministic(10, 3, seed=1))),
                      {"__class__": BRUE_AGENT, "step_strategy": "subtree"})


def test_exported_tree_objects():
    """build_brue_tree: DecisionNode / ChanceNode objects with the reference's keys (actions, str(observation))."""
    from rl_agents_amd.agents.tree_search.brue import ChanceNode, DecisionNode, build_brue_tree
    gen = np.random.Generator(np.random.PCG64(5))
    tab = generators.random_sparse(12, 3, 2, seed=4)
    res = br.brue_plan("sparse", tab["transition"], tab["reward"], tab["terminal"], 0, 40, 3, 0.8, gen, nxt=tab["next"])
    root = build_brue_tree(res)
    assert isinstance(root, DecisionNode) and root.depth == 0 and root.parent is None
    seen = 0
    for node, path in root.breadth_first_search(root):
        seen += 1
        for key, child in node.children.items():
            assert type(child) is (ChanceNode if isinstance(node, DecisionNode) else DecisionNode)
            assert isinstance(key, int if isinstance(node, DecisionNode) else str)
            assert child.depth == node.depth + (0 if isinstance(child, ChanceNode) else 1)
            assert child.path() == path + [key]
    assert seen == len(res["parent"])
    assert root.selection_rule() == int(res["plan"][0]) or res["ties"] > 1
