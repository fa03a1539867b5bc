"""BRUE on the device (mp_brue_plan, rl_agents_amd/csrc/brue.hip) against the reference's own outputs
(tests/golden/brue.npz) and the test-side restatement (tests/brue_restatement.py).

Parity: everything exactly -- plans, every tree array (the f64 running means by their bits), generator records, env-step
counts, get_visits and the error of a plan without a rollout."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.agents.tree_search.brue import ChanceNode
from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, generators
from tests import brue_restatement as br
from tests.test_brue_host import BRUE_AGENT, GOLDEN, generator_from, golden_case, names

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def env_of(tab, s0, available=None, max_steps=0, done_rule=None):
    cfg = dict(mode=str(tab["mode"]), transition=np.asarray(tab["transition"]).tolist(), reward=np.asarray(tab["reward"]).tolist(),
               terminal=np.asarray(tab["terminal"]).astype(int).tolist(), state=int(s0), max_steps=int(max_steps),
               done_rule=done_rule or tab.get("done_rule", "source"))
    if tab.get("next") is not None:
        cfg["next"] = np.asarray(tab["next"]).tolist()
    if available is not None and not np.asarray(available).all():
        env = MaskedFiniteMDPEnv(dict(cfg, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(cfg)
    env.reset()
    return env


def golden_table(case, prefix="mdp/"):
    return dict(mode=str(case[prefix + "mode"]), transition=case[prefix + "transition"], reward=case[prefix + "reward"],
                terminal=case[prefix + "terminal"], next=case.get(prefix + "next"))


def assert_tree(tree, ref, name):
    for k in br.TREE_KEYS:
        assert np.array_equal(tree[k], ref[k]), (name, k)
    assert np.array_equal(np.asarray(tree["stat"]).view(np.uint64), np.asarray(ref["stat"]).view(np.uint64)), (name, "stat bits")


def export_arrays(planner):
    """BFS listing (children in creation order) of the exported object tree, as the goldens list the reference's."""
    nodes, parents, keys = [planner.root], [-1], [-1]
    i = 0
    while i < len(nodes):
        for k, c in nodes[i].children.items():
            nodes.append(c)
            parents.append(i)
            keys.append(int(k))
        i += 1
    chance = [isinstance(n, ChanceNode) for n in nodes]
    return dict(parent=np.asarray(parents, np.int32), key=np.asarray(keys, np.int32), is_chance=np.asarray(chance, np.uint8),
                depth=np.asarray([n.depth for n in nodes], np.int32), count=np.asarray([n.count for n in nodes], np.int64),
                stat=np.asarray([n.value if c else n.reward for n, c in zip(nodes, chance)], np.float64))


def test_every_golden_case(z):
    checked = 0
    for name in names(z):
        case = golden_case(z, name)
        env = env_of(golden_table(case), int(case["s0"]), case["available"], int(case["max_steps"]),
                     "next" if bool(case["done_on_next"]) else "source")
        cfg = {"__class__": BRUE_AGENT, "budget": int(case["budget"]), "gamma": float(case["gamma"])}
        if bool(case["horizon_given"]):
            cfg["horizon"] = int(case["horizon"])
        agent = agent_factory(env, cfg)
        assert agent.planner.config["horizon"] == int(case["horizon"]), name
        native.generator_set_state(agent.planner.np_random, case["rng_before"])
        if str(case["error"]):
            with pytest.raises(ValueError):
                agent.plan(int(case["s0"]))
            assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
            assert agent.planner.env_steps == int(case["env_steps"]), name
            continue
        plan = agent.plan(int(case["s0"]))
        assert plan == case["plan"].tolist(), name
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
        assert agent.planner.env_steps == int(case["env_steps"]), name
        assert_tree(export_arrays(agent.planner), {k: case["tree/" + k] for k in br.TREE_KEYS}, name)
        visits = agent.planner.get_visits()
        assert sorted(visits) == [str(k) for k in case["visit_keys"]], name
        assert [visits[str(k)] for k in case["visit_keys"]] == case["visit_counts"].tolist(), name
        checked += 1
    assert checked >= 20


def test_act_episode_through_agent_factory(z):
    tab = golden_table({k[len("brue_episode/"):]: z[k] for k in z.files if k.startswith("brue_episode/")})
    env = env_of(tab, int(z["brue_episode/s0"]))
    env.seed(int(z["brue_episode/env_seed"]))
    agent = agent_factory(env, {"__class__": BRUE_AGENT, "budget": int(z["brue_episode/budget"]),
                                "gamma": float(z["brue_episode/gamma"])})
    agent.seed(int(z["brue_episode/seed"]))
    assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), z["brue_episode/rng_before"])
    for t in range(len(z["brue_episode/actions"])):
        assert env.mdp.state == int(z["brue_episode/states"][t])
        a = agent.act(env.mdp.state)
        assert a == int(z["brue_episode/actions"][t]), t
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), z["brue_episode/rng_after"][t]), t
        env.step(a)


def restated_root(tab, s0, pc, rng6, done_rule="source"):
    gen = generator_from(rng6)
    res = br.brue_plan(str(tab["mode"]), tab["transition"], tab["reward"], tab["terminal"], int(s0), int(pc["budget"]),
                       int(pc["horizon"]), float(pc["gamma"]), gen, nxt=tab.get("next"), done_rule=done_rule)
    return res, native.rng_state_from_generator(gen)


def check_batch(tab, cfg, roots, sample, tree_roots=(), done_rule="source"):
    env = env_of(tab, 0, done_rule=done_rule)
    agent = agent_factory(env, dict(cfg, __class__=BRUE_AGENT))
    planner = agent.planner
    rng = planner.batch_rng_states(len(roots))
    rng0 = rng.copy()
    out = planner.plan_batch(env, roots, rng_states=rng)
    assert (out["status"] == 0).all()
    for i in sample:
        res, rng_after = restated_root(tab, roots[i], planner.config, rng0[i], done_rule)
        assert out["plans"][i].tolist() == res["plan"].tolist(), i
        assert np.array_equal(rng[i], rng_after), i
        assert int(out["env_steps"][i]) == res["env_steps"], i
        assert np.float64(out["root_value"][i]).view(np.uint64) == np.float64(res["root_value"]).view(np.uint64), i
        if i in tree_roots:
            assert_tree(planner.models.ctx.brue_tree(i, planner._cap), res, i)
    return out, rng0, rng, planner


def test_fuzz_against_the_restatement():
    rng = np.random.default_rng(4321)
    modes = ["deterministic", "stochastic", "sparse"]
    for case in range(36):
        mode = modes[case % 3]
        S, A = int(rng.integers(2, 40)), int(rng.integers(1, 10))
        rate = float(rng.choice([0.0, 0.2, 0.5]))
        if mode == "deterministic":
            tab = generators.random_deterministic(S, A, seed=3000 + case, terminal_rate=rate)
        elif mode == "stochastic":
            tab = generators.random_stochastic(S, A, seed=3000 + case, terminal_rate=rate)
        else:
            tab = generators.random_sparse(S, A, int(rng.integers(1, 5)), seed=3000 + case, terminal_rate=rate)
        tab = dict(tab, mode=mode)
        if rng.random() < 0.3:
            tab["reward"] = (np.asarray(tab["reward"]) > 0.5).astype(np.float64)
        done_rule = "next" if (case // 3) % 2 else "source"
        cfg = {"gamma": float(rng.choice([0.5, 0.7, 0.8, 0.9, 0.95])), "budget": int(rng.integers(1, 601))}
        if rng.random() < 0.25:
            cfg["horizon"] = int(rng.integers(1, 12))
        n = int(rng.integers(1, 5))
        roots = rng.integers(0, S, size=n).astype(np.int32)
        check_batch(tab, cfg, roots, range(n), tree_roots=range(n), done_rule=done_rule)


@pytest.mark.parametrize("mode", ["sparse", "stochastic"])
def test_batch_of_4096_and_another_batch_composition(mode):
    if mode == "sparse":
        tab = dict(generators.random_sparse(200, 4, 3, seed=81, terminal_rate=0.05), mode=mode)
    else:
        tab = dict(generators.random_stochastic(48, 3, seed=82, terminal_rate=0.05), mode=mode)
    S = np.asarray(tab["reward"]).shape[0]
    cfg = {"gamma": 0.8, "budget": 300}
    n = 4096
    roots = (np.arange(n) * 37 % S).astype(np.int32)
    fixed = np.unique(np.concatenate([np.arange(0, n, 65), [n - 1]]))[:64]
    assert len(fixed) == 64
    out, rng0, rng, planner = check_batch(tab, cfg, roots, fixed.tolist(), tree_roots=(0, int(fixed[-1])))
    # the same roots with the same generator records, 64 of them in reverse order in a batch of their own
    env = env_of(tab, 0)
    other = agent_factory(env, dict(cfg, __class__=BRUE_AGENT)).planner
    sel = fixed[::-1].copy()
    rng_b = np.ascontiguousarray(rng0[sel])
    out_b = other.plan_batch(env, roots[sel], rng_states=rng_b)
    assert np.array_equal(out_b["plans"][:, 0], out["plans"][sel, 0])
    assert np.array_equal(out_b["env_steps"], out["env_steps"][sel])
    assert np.array_equal(out_b["root_value"].view(np.uint64), out["root_value"][sel].view(np.uint64))
    assert np.array_equal(rng_b, rng[sel])


def test_wide_nodes_and_workgroup_slots():
    """The 64-wide chunks of the kernel: more than 64 outcome children under one chance node (a dense model of 150 states
    with near-uniform rows and a single action), more than 64 actions, a dense row search over 150 thresholds; and a
    batch whose trees do not all fit the workspace (one tree slot per workgroup, root 0's kept for the export)."""
    wide = dict(generators.random_stochastic(150, 1, seed=91, concentration=50.0), mode="stochastic")
    check_batch(wide, {"gamma": 0.9, "budget": 500, "horizon": 2}, np.arange(6, dtype=np.int32), range(6), tree_roots=range(6))
    many = dict(generators.random_sparse(30, 70, 2, seed=92, terminal_rate=0.1), mode="sparse")
    check_batch(many, {"gamma": 0.8, "budget": 400}, (np.arange(8) * 3).astype(np.int32), range(8), tree_roots=range(8))
    ties = dict(generators.random_deterministic(20, 70, seed=93), mode="deterministic")
    ties["reward"] = np.zeros_like(np.asarray(ties["reward"]))           # 70 exact ties at the root: the tie draw
    check_batch(ties, {"gamma": 0.8, "budget": 90}, np.arange(8, dtype=np.int32), range(8), tree_roots=range(8))
    tab = dict(generators.random_sparse(100, 3, 2, seed=94), mode="sparse")
    n = 20000                                                            # 20 000 trees of 2 019 nodes: over the keep limit
    roots = (np.arange(n) * 7 % 100).astype(np.int32)
    out, _, _, planner = check_batch(tab, {"gamma": 0.8, "budget": 1000}, roots, [0, 1, 777, n - 1], tree_roots=(0,))
    assert planner.models.ctx.last_kernel_variant() == "brue_global_slots"
    with pytest.raises(native.NativeError):
        planner.models.ctx.brue_tree(1, planner._cap)


def test_refusals_and_tree_kinds():
    env = env_of(dict(generators.random_deterministic(10, 3, seed=1), mode="deterministic"), 0)
    with pytest.raises(NotImplementedError, match="subtree"):
        agent_factory(env, {"__class__": BRUE_AGENT, "step_strategy": "subtree"})
    agent = agent_factory(env, {"__class__": BRUE_AGENT, "budget": 0})
    with pytest.raises(ValueError):
        agent.act(0)
    ctx = native.Context(0)
    try:
        tab = generators.random_deterministic(20, 3, seed=7)
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        s0 = np.arange(4, dtype=np.int32)
        gp = np.array([0.8 ** d for d in range(4)])
        out = ctx.brue_plan(model, s0, 30, 3, 0.8, gp, native.seed_sequence_states((), 1, 4))
        assert (out["status"] == 0).all() and (out["plans"] >= 0).all()
        assert len(ctx.brue_tree(0, 1 + 2 * 33)["parent"]) > 1
        with pytest.raises(native.NativeError):
            ctx.olop_tree(0, 1 + 5 * 3 * 3)
        ctx.olop_plan(model, s0, 5, 3, 0.8, True, -1, np.full(5, 4 * np.log(5)),
                      np.array([(1 - 0.8 ** (4 - d)) / (1 - 0.8) for d in range(4)]), native.seed_sequence_states((), 2, 4))
        with pytest.raises(native.NativeError):
            ctx.brue_tree(0, 1 + 2 * 33)
        with pytest.raises(native.NativeError):
            ctx.brue_plan(model, s0, 30, 0, 0.8, np.array([1.0]), native.seed_sequence_states((), 1, 4))
        model.close()
    finally:
        ctx.close()
