"""Sparse Sampling on the host: the test-side restatement against the reference's own outputs
(tests/golden/sparse_sampling.npz), the positions of its draws in the raw stream, the node bound, the factories, the config
errors and the names of the forms -- no GPU needed."""
import os
import sys

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, generators
from tests import sparse_sampling_restatement as sr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sparse_sampling.npz")
SS_AGENT = "<class 'rl_agents_amd.agents.tree_search.sparse_sampling.SparseSamplingAgent'>"
REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def golden_case(z, name):
    p = "ss/" + name
    return {k[len(p) + 1:]: z[k] for k in z.files if k.startswith(p + "/")}


def names(z):
    return [str(n) for n in z["ss/names"]]


def generator_from(state6):
    gen = np.random.Generator(np.random.PCG64(0))
    native.generator_set_state(gen, np.asarray(state6, np.uint64))
    return gen


def listing_of(case):
    """(available, order) of a golden case as the restatement takes them: None where the env had no restriction."""
    if not bool(case["masked"]):
        return None, None
    return case["available"].astype(bool), case["order"]


def restate(case):
    """Run the restatement on one golden case's inputs; returns (result or the exception, generator after)."""
    gen = generator_from(case["rng_before"])
    available, order = listing_of(case)
    try:
        res = sr.ss_plan(str(case["mdp/mode"]), case["mdp/transition"], case["mdp/reward"], int(case["s0"]),
                         int(case["horizon"]), int(case["C"]), float(case["gamma"]), gen, nxt=case.get("mdp/next"),
                         available=available, order=order)
    except Exception as e:                  # (C = 0: the reference's own UnboundLocalError, restated)
        return e, gen
    return res, gen


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_restatement_equals_reference_goldens(z):
    checked = 0
    for name in names(z):
        case = golden_case(z, name)
        error = str(case["error"])
        assert int(case["env_steps"]) == 0, name                   # the samples never go through planner.step
        if error == "KeyError":             # a config without horizon or C: nothing to restate
            assert int(case["horizon"]) < 0 or int(case["C"]) < 0, name
            assert np.array_equal(case["rng_after"], case["rng_before"]), name
            continue
        res, gen = restate(case)
        assert np.array_equal(native.rng_state_from_generator(gen), case["rng_after"]), name
        if error:
            if error == "ValueError":
                assert res["error"] == "empty" and int(case["horizon"]) == 0, name
            else:
                assert type(res).__name__ == error == "UnboundLocalError" and int(case["C"]) == 0, name
            continue
        assert res["error"] is None, name
        assert int(case["n_visits"]) == 0, name
        assert np.array_equal(res["plan"], case["plan"]), name
        assert np.array_equal(res["root_actions"], case["root_actions"]), name
        assert np.array_equal(bits(res["root_values"]), bits(case["root_values"])), name
        tree = sr.as_bfs(res)
        for k in sr.TREE_KEYS:
            assert np.array_equal(tree[k], case["tree/" + k]), (name, k)
        assert np.array_equal(bits(tree["value"]), bits(case["tree/value"])), name   # by bits: the sign of zero too
        checked += 1
    assert checked >= 21


def test_goldens_cover_the_issue_cases(z):
    cases = {n: golden_case(z, n) for n in names(z)}
    planned = {n: c for n, c in cases.items() if not str(c["error"])}
    shipped = [c for c in planned.values() if (float(c["gamma"]), int(c["horizon"]), int(c["C"])) == (0.7, 3, 3)]
    assert {str(c["mdp/mode"]) for c in shipped} == {"deterministic", "stochastic", "sparse"}
    assert any(int(c["horizon"]) == 1 for c in planned.values())
    assert any(int(c["horizon"]) == 6 and int(c["C"]) == 1 and str(c["mdp/mode"]) == "deterministic" for c in planned.values())
    tied = [c for c in planned.values() if set(np.unique(c["mdp/reward"])) <= {0.0, 1.0}
            and np.count_nonzero(c["root_values"] == c["root_values"].max()) >= 2]
    assert tied and any(not np.array_equal(c["rng_after"], generator_after_draws(c)) for c in tied)
    assert any(c["mdp/reward"].shape[1] == 1 for c in planned.values())
    assert any(bool(c["masked"]) and not np.array_equal(c["order"], np.sort(c["order"])) for c in planned.values())
    assert any(c["mdp/reward"].min() < 0 and c["mdp/reward"].max() > 1 for c in planned.values())
    assert any((bits(c["mdp/reward"]) == bits([-0.0])[0]).any() for c in planned.values())
    for rule in (False, True):              # terminal states under both done rules, a root that is terminal, a step limit
        assert any(c["mdp/terminal"][int(c["s0"])] and bool(c["done_on_next"]) == rule for c in planned.values())
    assert any(c["mdp/terminal"].any() and not c["mdp/terminal"][int(c["s0"])] for c in planned.values())
    assert any(int(c["max_steps"]) > 0 for c in planned.values())
    assert any(int(c["C"]) % 2 and int(c["plans_before"]) and int(c["rng_before"][4]) == 1 for c in planned.values())
    c70 = cases["c70_dense"]
    assert int(c70["C"]) == 70 and int(c70["horizon"]) == 2 and c70["mdp/reward"].shape == (20, 3)
    wide = cases["list_over_64"]
    kids = np.bincount(wide["tree/parent"][1:], minlength=len(wide["tree/parent"]))
    recursed = (wide["tree/is_chance"] == 1) & (wide["tree/depth"] < int(wide["horizon"]) - 1)
    assert kids[recursed].max() > 64 and wide["mdp/reward"].shape == (100, 2) and int(wide["horizon"]) == 2
    assert {str(c["error"]) for c in cases.values()} == {"", "KeyError", "ValueError", "UnboundLocalError"}
    assert len(z["ss_episode/actions"]) == 6 and str(z["ss_episode/mdp/mode"]) == "sparse"


def generator_after_draws(case):
    """Record of the planner's generator after the plan's 30-bit draws alone (no tie draw)."""
    n = int(case["tree/count"].sum())       # one draw per sample; every sample is counted at one decision node
    gen = generator_from(case["rng_before"])
    if n:
        gen.integers(2 ** 30, size=n)
    return native.rng_state_from_generator(gen)


@pytest.mark.parametrize("buffered", [False, True])
def test_draw_i_is_one_half_word_of_the_raw_stream(buffered):
    """A 30-bit draw never rejects: draw i of a run is (half * 2**30) >> 32 of exactly one 32-bit half of the stream, the
    buffered half first, then low before high -- what lets lane i jump to its own draw."""
    gen = np.random.Generator(np.random.PCG64(1234))
    if buffered:
        gen.integers(7)                     # one 32-bit draw: the other half of its output stays buffered
    for n in (1, 2, 5, 64, 65, 151):
        record = native.rng_state_from_generator(gen)
        assert int(record[4]) == (1 if buffered else 0)
        words = sr.half_words(record, n + 1)
        following, words = words[n], words[:n]
        draws = [int(gen.integers(2 ** 30)) for _ in range(n)]
        assert draws == [(w << 30) >> 32 for w in words]
        after = native.rng_state_from_generator(gen)
        fresh = n - 1 if buffered else n
        assert int(after[4]) == fresh % 2
        buffered = bool(fresh % 2)
        if int(after[4]):
            assert int(after[5]) == following          # the unused high half stays in the record


def test_node_bound_covers_the_goldens(z):
    exact = 0
    for name in names(z):
        case = golden_case(z, name)
        if str(case["error"]):
            continue
        mode = str(case["mdp/mode"])
        n_actions, horizon, C = case["mdp/reward"].shape[1], int(case["horizon"]), int(case["C"])
        W = sr.max_outdegree(mode, case["mdp/transition"])
        g = native.ss_geometry(n_actions, horizon, C, W)
        assert g["list_entries"] == min(C, W)
        assert g["node_bound"] == sr.node_bound(n_actions, horizon, min(C, W)), name
        n_nodes = len(case["tree/parent"])
        assert g["node_bound"] >= n_nodes, name
        widest = np.bincount(case["tree/parent"][1:], minlength=n_nodes)[case["tree/is_chance"] == 1].max()
        assert widest <= g["list_entries"], name
        if mode == "deterministic" and not bool(case["masked"]):
            assert g["node_bound"] == n_nodes, name
            exact += 1
    assert exact >= 4
    assert native.ss_geometry(5, 16, 1024, 1024)["node_bound"] == -1      # beyond int32 indices
    for bad in ((3, 0, 3, 1), (3, 17, 3, 1), (3, 3, 0, 1), (3, 3, 1025, 1)):
        with pytest.raises(native.NativeError):
            native.ss_geometry(*bad)


def test_default_form_follows_the_frame_bytes(monkeypatch):
    monkeypatch.delenv("MP_SS_FRAMES", raising=False)
    small, big = native.ss_geometry(3, 3, 3, 3), native.ss_geometry(2, 16, 1024, 1024)
    assert small["lds"] and small["frame_bytes"] <= small["lds_limit"]
    assert not big["lds"] and big["frame_bytes"] > big["lds_limit"]


def grid_env():
    env = FiniteMDPEnv(generators.gridworld())
    env.reset()
    return env


def test_built_by_the_factories():
    from rl_agents_amd.agents.tree_search.sparse_sampling import SparseSampling, SparseSamplingAgent
    config = {"__class__": SS_AGENT, "gamma": 0.7, "horizon": 3, "C": 3}
    agent = agent_factory(grid_env(), dict(config))
    assert type(agent) is SparseSamplingAgent and type(agent.planner) is SparseSampling
    assert agent.planner.config["horizon"] == 3 and agent.planner.config["C"] == 3 and agent.planner.config["gamma"] == 0.7
    assert "horizon" not in SparseSampling.default_config() and "C" not in SparseSampling.default_config()
    assert agent.seed(3) == [3]
    assert dict(agent.planner.get_visits()) == {} and agent.planner.env_steps == 0
    if not os.path.isdir(REFERENCE):
        return
    # the reference's own factory builds this package's agent from the same JSON (gymnasium names through the test stubs)
    added = [os.path.join(HERE, "golden", "gen", "stubs"), REFERENCE]
    sys.path[:0] = added
    try:
        from rl_agents.agents.common.factory import agent_factory as reference_factory
        theirs = reference_factory(grid_env(), dict(config))
    finally:
        for p in added:
            sys.path.remove(p)
    assert type(theirs) is SparseSamplingAgent and theirs.planner.config["C"] == 3


def test_config_errors():
    for missing in ("horizon", "C"):
        config = {"__class__": SS_AGENT, "gamma": 0.7, "horizon": 3, "C": 3}
        del config[missing]
        agent = agent_factory(grid_env(), config)       # built without complaint: the keys are read at plan time
        before = native.rng_state_from_generator(agent.planner.np_random)
        with pytest.raises(KeyError, match=missing):
            agent.plan(0)
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), before)
    agent = agent_factory(grid_env(), {"__class__": SS_AGENT, "horizon": 0, "C": 3})
    with pytest.raises(ValueError, match="zero-size array"):
        agent.plan(0)
    agent = agent_factory(grid_env(), {"__class__": SS_AGENT, "horizon": 2, "C": 0})
    with pytest.raises(ValueError, match="C >= 1"):
        agent.plan(0)
    with pytest.raises(NotImplementedError, match="subtree"):
        agent_factory(grid_env(), {"__class__": SS_AGENT, "horizon": 2, "C": 2, "step_strategy": "subtree"})


def test_form_names():
    assert native.ss_form_names() == ["ss_wave_lds", "ss_wave_global"]
    listed = native.kernel_form_names()
    assert len(listed) == 172 and not any(n.startswith("ss_") for n in listed)     # the pinned list stays as it was
    assert "mp_ss_plan" in native.SIGNATURES and "mp_ss_tree_export" in native.SIGNATURES


def test_per_episode_evaluation_refuses_the_planner():
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    agent = agent_factory(grid_env(), {"__class__": SS_AGENT, "horizon": 2, "C": 2})
    with pytest.raises(NotImplementedError, match="one model per episode"):
        PerEpisodeEvaluation([grid_env(), grid_env()], agent)
