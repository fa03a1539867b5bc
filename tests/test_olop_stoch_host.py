"""OLOP / KL-OLOP on stochastic finite MDPs, on the host: the test-side restatement (tests/olop_stoch_restatement.py) against the
unmodified reference's own outputs (tests/golden/olop_stoch.npz), bit for bit in every array; what the fixture covers; the
two new entry points in the header, the signature table and the cross-compiled library; how ``OLOP.model_for`` loads a dense /
sparse model -- no GPU needed."""
import os
import re

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv
from tests import olop_restatement as olr
from tests import olop_stoch_restatement as osr
from tests.helpers import generator_from

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "olop_stoch.npz")
OLOP_AGENT = "<class 'rl_agents_amd.agents.tree_search.olop.StochasticOLOPAgent'>"
TABLE_AGENT = "<class 'rl_agents_amd.agents.tree_search.olop.OLOPAgent'>"
ERRORS = {"KeyError": "key", "ValueError": "range"}


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def names(z):
    return [str(n) for n in z["olop_stoch/names"]]


def golden_case(z, name):
    p = "olop_stoch/" + name
    return {k[len(p) + 1:]: z[k] for k in z.files if k.startswith(p + "/")}


def restate(case):
    """The restatement on one golden case's inputs -> (result, the planner's generator after)."""
    kl = str(case["bound_type"]) == "kullback-leibler"
    episodes, horizon = int(case["episodes"]), int(case["horizon"])
    thr = olr.thresholds(str(case["threshold"]), str(case["bound_time"]), episodes) if kl else None
    gen = generator_from(case["rng_before"])
    res = osr.olop_stoch_plan(str(case["mdp/mode"]), case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"],
                              int(case["s0"]), episodes, horizon, float(case["gamma"]), kl, thr, str(case["continuation"]), gen,
                              next_states=case.get("mdp/next"), available=case["available"] if bool(case["masked"]) else None,
                              order=case["order"], done_rule="next" if bool(case["done_on_next"]) else "source")
    return res, gen


def test_restatement_equals_the_reference_bit_for_bit(z):
    for name in names(z):
        case = golden_case(z, name)
        res, gen = restate(case)
        assert res["env_steps"] == int(case["env_steps"]), name
        assert np.array_equal(native.rng_state_from_generator(gen), case["rng_after"]), name
        assert ERRORS.get(str(case["error"])) == res["error"], name              # the same exception, or none
        assert np.array_equal(res["plan"], case["plan"]), name
        tree = olr.as_bfs(res)                                                   # (at the raise, where the reference raised)
        for k in ("parent", "action", "depth", "count", "done"):
            assert np.array_equal(tree[k], case["tree/" + k]), (name, k)
        for k in ("cum", "mu", "vu"):       # the restatement uses this host's numpy log, as the reference did: bit for bit
            assert np.array_equal(tree[k].view(np.uint64), case["tree/" + k].view(np.uint64)), (name, k)
        assert res["state"][0] == int(case["s0"]) and (res["state"][1:] == -1).all(), name


def test_the_fixture_covers_what_it_is_for(z):
    cases = {n: golden_case(z, n) for n in names(z)}
    planned = [c for c in cases.values() if not str(c["error"])]
    assert len(cases) == 14 and len(planned) == 12
    for c in cases.values():                                                     # small: the sizes the issue sets
        s, a = c["mdp/reward"].shape
        assert 4 <= s <= 12 and 2 <= a <= 3 and int(c["horizon"]) <= 6 and int(c["episodes"]) <= 60
    assert {str(c["mdp/mode"]) for c in planned} == {"stochastic", "sparse"}
    assert {c["mdp/transition"].shape[2] for c in planned if str(c["mdp/mode"]) == "sparse"} == {2, 3}
    assert {bool(c["done_on_next"]) for c in planned if c["tree/done"].any()} == {False, True}
    assert any(bool(c["late_done"]) and not bool(c["done_on_next"]) for c in planned)
    assert any(bool(c["late_done"]) and bool(c["done_on_next"]) for c in planned)
    kl = [c for c in planned if str(c["bound_type"]) == "kullback-leibler"]
    assert {str(c["bound_time"]) for c in kl} == {"global", "local"}
    assert {str(c["bound_type"]) for c in planned} >= {"kullback-leibler", "hoeffding", "laplace"}
    assert {str(c["continuation"]) for c in planned} == {"zeros", "uniform"}
    masked = [c for c in planned if bool(c["masked"])]
    assert any(bool(c["reentered"]) and np.array_equal(c["order"], np.arange(len(c["order"]))) for c in masked)
    assert any(bool(c["reentered"]) and not np.array_equal(c["order"], np.arange(len(c["order"]))) for c in masked)
    assert not any(bool(c["reentered"]) for c in planned if not bool(c["masked"]))
    key, rng = cases["masked_zeros_keyerror"], cases["reward_range"]
    assert str(key["error"]) == "KeyError" and int(key["horizon"]) < int(key["env_steps"]) < int(key["horizon"]) * int(key["episodes"])
    assert str(rng["error"]) == "ValueError" and int(rng["horizon"]) < int(rng["env_steps"]) < int(rng["horizon"]) * int(rng["episodes"])
    assert any((c["mdp/reward"] == 0).any() and (c["mdp/reward"] == 1).any() for c in planned)


def test_header_signatures_and_library_have_the_entry_points():
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    assert re.search(r"\bint mp_olop_plan_stochastic\(mp_ctx \*ctx, mp_model \*model, int32_t n_roots", header)
    assert re.search(r"\bconst char \*mp_olop_stoch_form_names\(void\);", header)
    assert re.search(r"#define\s+MP_ABI_VERSION\s+7\b", header)
    for symbol in ("mp_olop_plan_stochastic", "mp_olop_stoch_form_names"):
        assert symbol in native.SIGNATURES, symbol
    # arguments, host tables, mem flag and outputs are those of mp_olop_plan
    assert native.SIGNATURES["mp_olop_plan_stochastic"] == native.SIGNATURES["mp_olop_plan"]
    lib = native.load()
    assert lib.mp_abi_version() == 7
    assert lib.mp_olop_plan_stochastic is not None and lib.mp_olop_stoch_form_names is not None
    form_names = native.olop_stoch_form_names()
    assert form_names == ["olop_stoch_dense", "olop_stoch_sparse"]
    assert lib.mp_olop_stoch_form_names() == b"olop_stoch_dense\nolop_stoch_sparse"
    for other in (native.kernel_form_names(), native.each_form_names(), native.ss_form_names(), native.ss_each_form_names()):
        assert not set(form_names) & set(other)


class RecordingModel(object):
    mode = native.MODE_SPARSE

    def __init__(self):
        self.calls = []

    def set_available(self, available):
        self.calls.append(("available", np.array(available)))
        self.available = np.asarray(available).astype(bool)

    def set_episode_rules(self, done_rule, max_steps):
        self.calls.append(("rules", done_rule, max_steps))


class RecordingCache(object):
    def __init__(self):
        self.specs, self.model = [], RecordingModel()

    def get(self, spec):
        self.specs.append(spec)
        return self.model


def sparse_env(cls, z, **extra):
    case = golden_case(z, "ordered_sparse_kl_uniform")
    cfg = dict(mode="sparse", transition=case["mdp/transition"].tolist(), next=case["mdp/next"].tolist(),
               reward=case["mdp/reward"].tolist(), terminal=case["mdp/terminal"].astype(int).tolist(), done_rule="next", **extra)
    env = cls(cfg)
    env.reset()
    return env, case


def test_model_for_loads_a_stochastic_model_with_the_envs_listing(z):
    """OLOP.model_for on a sparse env: the spec carries the env's availability table, its columns in the listing order; the
    model gets the table once, and the env's done rule with no step limit at every call."""
    env, case = sparse_env(OrderedMaskedFiniteMDPEnv, z, available=case_available(z), listing_order=[2, 0, 1])
    planner = agent_factory(env, {"__class__": OLOP_AGENT, "budget": 30}).planner
    planner.models = cache = RecordingCache()
    for _ in range(2):
        assert planner.model_for(env) is cache.model
    spec = cache.specs[0]
    assert spec.mode == "sparse" and spec.action_order.tolist() == [2, 0, 1] and spec.done_rule == "next"
    assert np.array_equal(spec.available.astype(bool), case["available"][:, [2, 0, 1]])
    assert np.array_equal(spec.transition, case["mdp/transition"][:, [2, 0, 1]])
    kinds = [c[0] for c in cache.model.calls]
    assert kinds == ["available", "rules", "rules"]
    assert np.array_equal(cache.model.calls[0][1], spec.available)
    assert cache.model.calls[1][1:] == ("next", 0)


def case_available(z):
    return golden_case(z, "ordered_sparse_kl_uniform")["available"].astype(int).tolist()


def test_model_for_without_a_listing_sets_no_table(z):
    env, _ = sparse_env(FiniteMDPEnv, z)
    planner = agent_factory(env, {"__class__": OLOP_AGENT, "budget": 30}).planner
    planner.models = cache = RecordingCache()
    planner.model_for(env)
    assert cache.specs[0].available is None and cache.specs[0].action_order is None
    assert [c[0] for c in cache.model.calls] == ["rules"]
    masked, case = sparse_env(MaskedFiniteMDPEnv, z, available=case_available(z))
    planner.models = cache = RecordingCache()
    planner.model_for(masked)
    assert np.array_equal(cache.specs[0].available.astype(bool), case["available"]) and cache.specs[0].action_order is None


def test_olop_agent_keeps_its_refusal_and_the_new_agent_its_tables(z):
    """OLOPAgent behaves as it always has: the base class's TypeError on a sparse env, before any model is asked for.
    StochasticOLOPAgent is the same planner with the one switch set, and on a deterministic env takes the base class's route."""
    from rl_agents_amd.agents.tree_search.olop import OLOP, OLOPAgent, StochasticOLOP, StochasticOLOPAgent
    from rl_agents_amd.envs import generators
    env, _ = sparse_env(FiniteMDPEnv, z)
    planner = agent_factory(env, {"__class__": TABLE_AGENT, "budget": 30}).planner
    planner.models = cache = RecordingCache()
    with pytest.raises(TypeError, match="deterministic"):
        planner.model_for(env)
    assert not cache.specs and type(planner) is OLOP and not OLOP.accepts_stochastic_models
    assert issubclass(StochasticOLOP, OLOP) and StochasticOLOPAgent.PLANNER_TYPE is StochasticOLOP and OLOPAgent.PLANNER_TYPE is OLOP
    assert {k for k, v in vars(StochasticOLOP).items() if not k.startswith("__")} == {"accepts_stochastic_models"}
    table = FiniteMDPEnv(dict(generators.random_deterministic(10, 3, seed=1)))
    specs = []
    for agent_class in (TABLE_AGENT, OLOP_AGENT):
        planner = agent_factory(table, {"__class__": agent_class, "budget": 30}).planner
        planner.models = cache = RecordingCache()
        planner.model_for(table)
        assert cache.model.calls == []                      # a table gets its rules and flags at its upload
        specs.append(cache.specs[0])
    assert specs[0].key() == specs[1].key() and specs[0].mode == "deterministic"


def test_subtree_stays_refused_on_a_stochastic_env(z):
    env, _ = sparse_env(FiniteMDPEnv, z)
    with pytest.raises(NotImplementedError):
        agent_factory(env, {"__class__": OLOP_AGENT, "step_strategy": "subtree"})


def test_an_export_of_a_stochastic_tree_has_no_state_below_the_root():
    from rl_agents_amd.agents.tree_search.olop import build_olop_tree
    arrays = dict(parent=np.array([-1, 0, 0]), action=np.array([-1, 0, 1]), count=np.array([0, 2, 1]), depth=np.array([0, 1, 1]),
                  vu=np.array([3.0, 2.0, 1.0]), mu=np.ones(3), cum=np.zeros(3), done=np.zeros(3, np.uint8), state=np.array([4, -1, -1]))
    root = build_olop_tree(arrays)
    assert root.state == 4 and [c.state for c in root.children.values()] == [None, None]
    assert root.selection_rule() == 0
