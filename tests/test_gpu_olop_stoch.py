"""OLOP / KL-OLOP on stochastic finite MDPs on the device (mp_olop_plan_stochastic, rl_agents_amd/csrc/olop.hip) against the
unmodified reference's own outputs (tests/golden/olop_stoch.npz), the test-side restatement (tests/olop_stoch_restatement.py)
and, on one-hot models, mp_olop_plan itself.

Parity: plans, tree shapes, actions, counts, done flags, cumulative rewards, generator records, env-step counts and the status /
exception exactly; mu_ucb, value_upper and root_value within 1e-12 (the device's log in the KL bound's Newton step)
-- bit for bit against mp_olop_plan, which runs the same device code."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.common.factory import agent_factory
from rl_agents_amd.agents.tree_search.olop import OLOP, OLOPNode
from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv, generators
from tests import olop_restatement as olr
from tests import olop_stoch_restatement as osr
from tests.helpers import generator_from
from tests.test_gpu_olop import assert_tree, export_arrays
from tests.test_olop_stoch_host import ERRORS, GOLDEN, OLOP_AGENT, golden_case, names

pytestmark = pytest.mark.gpu

BOUND_TOL = 1e-12
STATUS = {None: native.MP_OK, "key": native.ERR_OLOP_KEY, "range": native.MP_ERR_REWARD_RANGE}
KL = dict(type="kullback-leibler", time="global", threshold="4*np.log(time)")


@pytest.fixture(scope="module")
def ctx():
    return native.Context(0)


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def load_model(ctx, cfg, available=None, order=None, done_rule="source"):
    """A dense / sparse model as OLOP.model_for loads it: columns in the env's listing order, the availability table, the done
    rule with no step limit."""
    order = np.arange(np.asarray(cfg["reward"]).shape[1]) if order is None else np.asarray(order)
    t, r = np.asarray(cfg["transition"])[:, order], np.asarray(cfg["reward"])[:, order]
    if cfg["mode"] == "sparse":
        model = ctx.load_sparse(t, np.asarray(cfg["next"])[:, order], r, cfg.get("terminal"))
    else:
        model = ctx.load_dense(t, r, cfg.get("terminal"))
    if available is not None:
        model.set_available(np.asarray(available)[:, order])
    model.set_episode_rules(done_rule, 0)
    return model


def continuation_label(continuation, order=None):
    if continuation == "uniform":
        return -1
    return 0 if order is None else [int(a) for a in order].index(0)


def plan_call(ctx, model, roots, episodes, horizon, gamma, kl, thr, label, rng):
    out = ctx.olop_plan_stochastic(model, roots, episodes, horizon, gamma, kl, label, thr if kl else np.zeros(0),
                                   OLOP.value_upper_init(gamma, horizon), rng)
    assert ctx.last_kernel_variant() == ("olop_stoch_sparse" if model.mode == native.MODE_SPARSE else "olop_stoch_dense")
    assert ctx.last_kernel_variant() in native.olop_stoch_form_names()
    return out


def device_tree(ctx, root, episodes, horizon, n_actions, order=None):
    tree = ctx.olop_tree(root, 1 + episodes * horizon * n_actions)
    if order is not None:
        act = tree["action"]
        tree["action"] = np.where(act >= 0, np.asarray(order)[np.maximum(act, 0)], act).astype(act.dtype)
    return tree


def assert_close(got, want, what):
    if np.isfinite(want):
        assert abs(got - want) <= BOUND_TOL, what
    else:
        assert np.array_equal(got, want, equal_nan=True), what


def case_config(case):
    kl = str(case["bound_type"]) == "kullback-leibler"
    episodes, horizon = int(case["episodes"]), int(case["horizon"])
    thr = olr.thresholds(str(case["threshold"]), str(case["bound_time"]), episodes) if kl else None
    return kl, episodes, horizon, thr


def case_mdp(case):
    cfg = dict(mode=str(case["mdp/mode"]), transition=case["mdp/transition"], reward=case["mdp/reward"], terminal=case["mdp/terminal"])
    if cfg["mode"] == "sparse":
        cfg["next"] = case["mdp/next"]
    return cfg


def case_model(ctx, case):
    order = case["order"]
    return load_model(ctx, case_mdp(case), case["available"] if bool(case["masked"]) else None, order,
                      "next" if bool(case["done_on_next"]) else "source")


def golden_tree(case):
    return {k: case["tree/" + k] for k in ("parent", "action", "depth", "count", "cum", "mu", "vu", "done")}


# ------------------------------------------------------------------------------------------- 1. the reference's own outputs
def test_every_golden_case_through_the_context(ctx, z):
    for name in names(z):
        case = golden_case(z, name)
        kl, episodes, horizon, thr = case_config(case)
        model = case_model(ctx, case)
        rng = case["rng_before"].reshape(1, 6).copy()
        label = continuation_label(str(case["continuation"]), case["order"])
        out = plan_call(ctx, model, [int(case["s0"])], episodes, horizon, float(case["gamma"]), kl, thr, label, rng)
        assert int(out["status"][0]) == STATUS[ERRORS.get(str(case["error"]))], name
        assert int(out["env_steps"][0]) == int(case["env_steps"]), name
        assert np.array_equal(rng[0], case["rng_after"]), name
        if str(case["error"]):
            assert int(out["plan_len"][0]) == 0 and (out["plans"] == -1).all(), name
            model.close()
            continue
        n = int(out["plan_len"][0])
        assert case["order"][out["plans"][0, :n]].tolist() == case["plan"].tolist(), name
        tree = device_tree(ctx, 0, episodes, horizon, model.A, case["order"])
        assert int(tree["state"][0]) == int(case["s0"]) and (tree["state"][1:] == -1).all(), name
        assert_tree(olr.as_bfs(tree), golden_tree(case), name)
        assert_close(out["root_value"][0], case["tree/vu"][0], name)
        model.close()


def env_of(cfg, s0, available=None, order=None, done_rule="source"):
    c = {k: (np.asarray(v).tolist() if not isinstance(v, str) else v) for k, v in cfg.items() if v is not None}
    c.update(state=int(s0), max_steps=0, done_rule=done_rule)
    if "terminal" in c:
        c["terminal"] = np.asarray(cfg["terminal"]).astype(int).tolist()
    if available is not None and order is not None and not np.array_equal(order, np.arange(len(order))):
        env = OrderedMaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist(),
                                             listing_order=[int(a) for a in order]))
    elif available is not None:
        env = MaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def case_agent(case):
    env = env_of(case_mdp(case), int(case["s0"]), case["available"] if bool(case["masked"]) else None, case["order"],
                 "next" if bool(case["done_on_next"]) else "source")
    cfg = dict(gamma=float(case["gamma"]), continuation_type=str(case["continuation"]),
               upper_bound=dict(type=str(case["bound_type"]), time=str(case["bound_time"]), threshold=str(case["threshold"])),
               episodes=int(case["episodes"]), horizon=int(case["horizon"]))
    agent = agent_factory(env, dict(cfg, __class__=OLOP_AGENT))
    native.generator_set_state(agent.planner.np_random, case["rng_before"])
    return agent


def test_every_golden_case_through_the_agent(z):
    for name in names(z):
        case = golden_case(z, name)
        agent = case_agent(case)
        if str(case["error"]):
            with pytest.raises({"KeyError": KeyError, "ValueError": ValueError}[str(case["error"])]):
                agent.plan(int(case["s0"]))
        else:
            assert agent.plan(int(case["s0"])) == case["plan"].tolist(), name
            assert_tree(export_arrays(agent.planner), golden_tree(case), name)
            assert_close(agent.planner.last["root_value"][0], case["tree/vu"][0], name)
        # (the draws and steps made before the reference raised, where it raised)
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
        assert agent.planner.env_steps == int(case["env_steps"]), name
        assert agent.planner.models.ctx.last_kernel_variant() in native.olop_stoch_form_names(), name


def test_get_visits_is_refused_and_the_exported_tree_reproduces_the_plan(z):
    case = golden_case(z, "ordered_sparse_kl_uniform")
    agent = case_agent(case)
    plan = agent.plan(int(case["s0"]))
    with pytest.raises(NotImplementedError, match="no single"):
        agent.planner.get_visits()
    root = agent.planner.export_tree(0)
    assert isinstance(root, OLOPNode) and root.state == int(case["s0"])
    node, walked = root, []
    while node.children:
        action = node.selection_rule()
        walked.append(action)
        node = node.children[action]
        assert isinstance(node, OLOPNode) and node.state is None
    assert walked == plan == case["plan"].tolist()


# ------------------------------------------------------------------------------------------- 2. one-hot models = the table
def one_hot_models(ctx, table, available, done_rule):
    t, r, term = np.asarray(table["transition"]), np.asarray(table["reward"]), np.asarray(table["terminal"])
    n_states, n_actions = r.shape
    dense = np.zeros((n_states, n_actions, n_states))
    np.put_along_axis(dense, t[:, :, None], 1.0, axis=2)
    nxt = np.stack([(t + 1) % n_states, t, (t + 3) % n_states], axis=2)            # the table's successor in the middle
    prob = np.zeros((n_states, n_actions, 3))
    prob[:, :, 1] = 1.0
    return (ctx.load_table(t, r, term, done_rule=done_rule, available=available),
            load_model(ctx, dict(mode="stochastic", transition=dense, reward=r, terminal=term), available, None, done_rule),
            load_model(ctx, dict(mode="sparse", transition=prob, next=nxt, reward=r, terminal=term), available, None, done_rule))


@pytest.mark.parametrize("n_actions", [3, 70])
def test_one_hot_models_give_what_the_table_gives_bit_for_bit(ctx, n_actions):
    """Rows that put probability 1 on the table's successor: the same device code as mp_olop_plan, so everything is compared by
    bits, the bounds included.  |A| = 70 walks the 64-wide child loops twice."""
    n_states, gamma = 8, 0.8
    episodes, horizon = OLOP.allocation(max(60, n_actions), gamma)
    for k, (continuation, done_rule) in enumerate([("uniform", "source"), ("zeros", "next")]):
        table = generators.random_deterministic(n_states, n_actions, seed=300 + n_actions + k, terminal_rate=0.25)
        available = generators.random_available(n_states, n_actions, seed=310 + k, rate=0.3)
        available[:, 0] = True
        thr = olr.thresholds(KL["threshold"], "global", episodes)
        roots = np.arange(n_states, dtype=np.int32)
        vinit = OLOP.value_upper_init(gamma, horizon)
        label = continuation_label(continuation)
        results = []
        for model in one_hot_models(ctx, table, available, done_rule):
            rng = native.seed_sequence_states([77 + k], 0, n_states)
            if model.mode == native.MODE_DETERMINISTIC:
                out = ctx.olop_plan(model, roots, episodes, horizon, gamma, True, label, thr, vinit, rng)
                assert ctx.last_kernel_variant() == "olop_global"
            else:
                out = plan_call(ctx, model, roots, episodes, horizon, gamma, True, thr, label, rng)
            trees = [device_tree(ctx, i, episodes, horizon, n_actions) for i in (0, n_states - 1)]
            results.append((out, rng, trees))
            model.close()
        (want, want_rng, want_trees) = results[0]
        assert (want["status"] == native.MP_OK).all() and (want["env_steps"] == episodes * horizon).all()
        for out, rng, trees in results[1:]:
            for key in ("plans", "plan_len", "env_steps", "status"):
                assert np.array_equal(out[key], want[key]), key
            assert np.array_equal(out["root_value"].view(np.uint64), want["root_value"].view(np.uint64))
            assert np.array_equal(rng, want_rng)
            for tree, ref in zip(trees, want_trees):
                for key in ("parent", "action", "depth", "count", "done"):
                    assert np.array_equal(tree[key], ref[key]), key
                for key in ("cum", "mu", "vu"):
                    assert np.array_equal(tree[key].view(np.uint64), ref[key].view(np.uint64)), key


# ------------------------------------------------------------------------------------------- 3. against the restatement
def restated(cfg, s0, episodes, horizon, gamma, kl, thr, continuation, rng6, available=None, order=None, done_rule="source"):
    gen = generator_from(rng6)
    res = osr.olop_stoch_plan(cfg["mode"], cfg["transition"], cfg["reward"], cfg.get("terminal"), int(s0), episodes, horizon, gamma,
                              kl, thr, continuation, gen, next_states=cfg.get("next"), available=available, order=order,
                              done_rule=done_rule)
    return res, native.rng_state_from_generator(gen)


def assert_root(out, rng, i, res, rng_after, what, order=None):
    assert int(out["status"][i]) == STATUS[res["error"]], what
    assert int(out["env_steps"][i]) == res["env_steps"], what
    assert np.array_equal(rng[i], rng_after), what
    n = int(out["plan_len"][i])
    plan = out["plans"][i, :n] if order is None else np.asarray(order)[out["plans"][i, :n]]
    assert plan.tolist() == res["plan"].tolist(), what
    if res["error"] is None:
        assert_close(out["root_value"][i], res["vu"][0], what)


@pytest.mark.parametrize("kind,n_states", [("stochastic", 70), ("stochastic", 130), ("sparse", 40)])
def test_row_search_wider_than_a_ballot(ctx, kind, n_states):
    """Dense rows of 70 and 130 thresholds: two and three ballots a step, the successors spread over the whole row (the Dirichlet
    rows of the generator); sparse rows of B = 3."""
    if kind == "sparse":
        cfg = generators.random_sparse(n_states, 3, 3, seed=400, terminal_rate=0.1)
    else:
        cfg = generators.random_stochastic(n_states, 2, seed=400 + n_states, terminal_rate=0.1, concentration=1.0)
    episodes, horizon, gamma = 30, 3, 0.8
    thr = olr.thresholds(KL["threshold"], "global", episodes)
    roots = np.asarray([0, 1, n_states // 2, n_states - 1], np.int32)
    rng = native.seed_sequence_states([5], 0, len(roots))
    rng0 = rng.copy()
    model = load_model(ctx, cfg)
    out = plan_call(ctx, model, roots, episodes, horizon, gamma, True, thr, -1, rng)
    if kind == "stochastic":        # every row has mass past its last full ballot (and so past the first, at 130)
        assert cfg["transition"][:, :, 64 * ((n_states - 1) // 64):].sum(axis=2).min() > 0
    for i, s0 in enumerate(roots):
        res, rng_after = restated(cfg, s0, episodes, horizon, gamma, True, thr, "uniform", rng0[i])
        assert_root(out, rng, i, res, rng_after, (kind, n_states, i))
        assert_tree(device_tree(ctx, i, episodes, horizon, model.A), res, (kind, n_states, i))
    model.close()


def sweep_case(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    n_states, n_actions = int(g.integers(2, 21)), int(g.integers(1, 7))
    terminal_rate = float(g.choice([0.0, 0.2, 0.5]))
    if g.random() < 0.5:
        cfg = generators.random_stochastic(n_states, n_actions, seed=seed, terminal_rate=terminal_rate)
    else:
        cfg = generators.random_sparse(n_states, n_actions, int(g.integers(1, 5)), seed=seed, terminal_rate=terminal_rate)
    reward = np.asarray(cfg["reward"]).copy()
    reward[reward < 0.2] = 0.0                                                     # exact 0 and 1 among the rewards
    reward[reward > 0.8] = 1.0
    cfg["reward"] = reward
    available = generators.random_available(n_states, n_actions, seed=seed + 1, rate=float(g.choice([0.0, 0.3, 0.6])))
    order = g.permutation(n_actions) if g.random() < 0.5 else None
    shape = [(0, 3), (1, 1), (1, 4), (7, 1), (12, 3), (25, 4), (40, 2), (30, 6)][int(g.integers(0, 8))]
    bound = [KL, dict(KL, time="local", threshold="2*np.log(time)"), dict(type="hoeffding")][int(g.integers(0, 3))]
    return dict(cfg=cfg, available=available, order=order, episodes=shape[0], horizon=shape[1], bound=bound,
                continuation="uniform" if g.random() < 0.6 else "zeros", done_rule="next" if g.random() < 0.5 else "source",
                gamma=float(g.choice([0.5, 0.8, 0.95])), s0=int(g.integers(0, n_states)))


def test_fixed_seed_sweep_against_the_restatement(ctx):
    seen = dict(key=0, ok=0, episodes=set(), horizons=set(), rules=set(), modes=set())
    for seed in range(5000, 5040):
        c = sweep_case(seed)
        kl = c["bound"]["type"] == "kullback-leibler"
        thr = olr.thresholds(c["bound"]["threshold"], c["bound"]["time"], c["episodes"]) if kl else None
        model = load_model(ctx, c["cfg"], c["available"], c["order"], c["done_rule"])
        rng = native.seed_sequence_states([seed], 0, 1)
        rng0 = rng.copy()
        label = continuation_label(c["continuation"], c["order"])
        out = plan_call(ctx, model, [c["s0"]], c["episodes"], c["horizon"], c["gamma"], kl, thr, label, rng)
        res, rng_after = restated(c["cfg"], c["s0"], c["episodes"], c["horizon"], c["gamma"], kl, thr, c["continuation"], rng0[0],
                                  c["available"], c["order"], c["done_rule"])
        what = "sweep case of seed {}".format(seed)
        assert_root(out, rng, 0, res, rng_after, what, c["order"])
        if res["error"] is None:
            assert_tree(device_tree(ctx, 0, c["episodes"], c["horizon"], model.A, c["order"]), res, what)
        seen["key" if res["error"] else "ok"] += 1
        seen["episodes"].add(c["episodes"]); seen["horizons"].add(c["horizon"]); seen["rules"].add(c["done_rule"])
        seen["modes"].add(c["cfg"]["mode"])
        model.close()
    assert seen["ok"] >= 25 and {0, 1} <= seen["episodes"] and 1 in seen["horizons"], seen
    assert seen["rules"] == {"source", "next"} and seen["modes"] == {"stochastic", "sparse"}, seen


def test_more_roots_than_workgroups_and_the_kept_trees(ctx):
    """10 000 roots: more than the launch has workgroups (32 a compute unit), every root against the restatement; the call
    again, and the trees of root 0 and of the last root, all kept (a tree of 17 nodes a root)."""
    cfg = dict(generators.random_sparse(4, 2, 2, seed=500), terminal=np.array([False, True, False, False]))
    n, episodes, horizon, gamma = 10000, 4, 2, 0.8
    assert n > ctx.device_info()["n_cu"] * 32
    thr = olr.thresholds(KL["threshold"], "global", episodes)
    roots = (np.arange(n) % 4).astype(np.int32)
    model = load_model(ctx, cfg)
    rng0 = native.seed_sequence_states([9], 0, n)
    refs = [restated(cfg, roots[i], episodes, horizon, gamma, True, thr, "uniform", rng0[i]) for i in range(n)]
    for _ in range(2):
        rng = rng0.copy()
        out = plan_call(ctx, model, roots, episodes, horizon, gamma, True, thr, -1, rng)
        assert (out["status"] == native.MP_OK).all() and (out["env_steps"] == episodes * horizon).all()
        assert np.array_equal(rng, np.stack([r[1] for r in refs]))
        assert np.array_equal(out["plan_len"], [len(r[0]["plan"]) for r in refs])
        for i in range(n):
            assert out["plans"][i, :out["plan_len"][i]].tolist() == refs[i][0]["plan"].tolist(), i
        assert np.abs(out["root_value"] - np.asarray([r[0]["vu"][0] for r in refs])).max() <= BOUND_TOL
    for i in (0, n - 1):
        assert_tree(device_tree(ctx, i, episodes, horizon, model.A), refs[i][0], i)
    model.close()


# ------------------------------------------------------------------------------------------- 4. device arrays, refusals
def test_device_arrays_give_what_host_arrays_give(ctx, z):
    import torch
    case = golden_case(z, "masked_sparse_kl_local_uniform")
    kl, episodes, horizon, thr = case_config(case)
    model = case_model(ctx, case)
    n = 5
    roots = (np.arange(n) % case["mdp/reward"].shape[0]).astype(np.int32)
    roots[0] = int(case["s0"])
    rng0 = np.concatenate([case["rng_before"].reshape(1, 6), native.seed_sequence_states([3], 0, n - 1)])
    rng = rng0.copy()
    want = plan_call(ctx, model, roots, episodes, horizon, float(case["gamma"]), kl, thr, -1, rng)
    assert np.array_equal(rng[0], case["rng_after"])
    want_tree = device_tree(ctx, 0, episodes, horizon, model.A)
    dev = torch.device("cuda", ctx.device)
    d = dict(s0=torch.from_numpy(roots).to(dev), rng=torch.from_numpy(rng0.view(np.int64).copy()).to(dev),
             plans=torch.full((n, horizon), -7, dtype=torch.int32, device=dev), plan_len=torch.zeros(n, dtype=torch.int32, device=dev),
             value=torch.zeros(n, dtype=torch.float64, device=dev), steps=torch.zeros(n, dtype=torch.int64, device=dev),
             status=torch.full((n,), -1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ptr = native._ptr
    vinit = OLOP.value_upper_init(float(case["gamma"]), horizon)
    native._check(ctx._lib.mp_olop_plan_stochastic(ctx._h, model._h, n, ptr(d["s0"]), episodes, horizon, float(case["gamma"]), 1, -1,
                                                   ptr(thr), ptr(vinit), ptr(d["rng"]), horizon, ptr(d["plans"]), ptr(d["plan_len"]),
                                                   ptr(d["value"]), ptr(d["steps"]), ptr(d["status"]), native.MP_MEM_DEVICE))
    assert ctx.last_kernel_variant() == "olop_stoch_sparse"
    ctx.synchronize()
    assert np.array_equal(d["rng"].cpu().numpy().view(np.uint64), rng)
    for key, name in (("plans", "plans"), ("plan_len", "plan_len"), ("steps", "env_steps"), ("status", "status")):
        assert np.array_equal(d[key].cpu().numpy(), want[name]), key
    assert np.array_equal(d["value"].cpu().numpy().view(np.uint64), want["root_value"].view(np.uint64))
    tree = device_tree(ctx, 0, episodes, horizon, model.A)
    for key in tree:
        assert np.array_equal(tree[key], want_tree[key], equal_nan=True), key
    model.close()


def test_refusals(ctx):
    table = generators.random_deterministic(6, 2, seed=1)
    dense = generators.random_stochastic(6, 2, seed=2)
    det = ctx.load_table(table["transition"], table["reward"], table["terminal"])
    batch = ctx.load_table_batch(np.stack([table["transition"]] * 2), np.stack([table["reward"]] * 2))
    stoch = load_model(ctx, dense)
    thr, vinit = np.full(3, 4 * np.log(3)), OLOP.value_upper_init(0.8, 2)
    for model in (det, batch):
        with pytest.raises(native.NativeError) as e:
            ctx.olop_plan_stochastic(model, [0], 3, 2, 0.8, True, -1, thr, vinit, native.seed_sequence_states([1], 0, 1))
        assert e.value.code == native.MP_ERR_MODE and "mp_olop_plan" in str(e.value)
    with pytest.raises(native.NativeError) as e:               # mp_olop_plan keeps refusing a dense model
        ctx.olop_plan(stoch, [0], 3, 2, 0.8, True, -1, thr, vinit, native.seed_sequence_states([1], 0, 1))
    assert e.value.code == native.MP_ERR_MODE
    rng = native.seed_sequence_states([1], 0, 1)
    out = plan_call(ctx, stoch, [0], 3, 2, 0.8, True, thr, -1, rng)
    assert int(out["status"][0]) == native.MP_OK and int(out["env_steps"][0]) == 6
    for model in (det, batch, stoch):
        model.close()


def test_on_tables_the_new_agent_is_olop_agent_and_olop_agent_still_refuses(z):
    """StochasticOLOPAgent on deterministic tables: the reference's own outputs of tests/golden/olop.npz, through mp_olop_plan.
    OLOPAgent on a dense env: the TypeError it has always raised."""
    from tests import test_gpu_olop as table_tests
    from tests import test_olop_host as table_host
    zt = np.load(table_host.GOLDEN)
    for name in ("fmdp_kl_global", "ordered_kl_uniform", "done_next_kl"):
        case = table_host.golden_case(zt, name)
        agent = agent_factory(table_tests.golden_env(case), dict(table_tests.agent_config(case), __class__=OLOP_AGENT))
        native.generator_set_state(agent.planner.np_random, case["rng_before"])
        assert agent.plan(int(case["s0"])) == case["plan"].tolist(), name
        assert agent.planner.models.ctx.last_kernel_variant() == "olop_global", name
        assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), case["rng_after"]), name
        ref = {k: case["tree/" + k] for k in ("parent", "action", "depth", "count", "cum", "mu", "vu", "done")}
        assert_tree(export_arrays(agent.planner), ref, name)
        visits = agent.planner.get_visits()
        assert [visits[str(k)] for k in case["visit_keys"]] == case["visit_counts"].tolist(), name
    case = golden_case(z, "dense_kl_global_uniform")
    env = env_of(case_mdp(case), int(case["s0"]))
    agent = agent_factory(env, {"__class__": table_host.OLOP_AGENT, "budget": 50})
    with pytest.raises(TypeError, match="deterministic"):
        agent.plan(int(case["s0"]))


def test_a_reference_config_with_only_its_class_line_changed():
    """SailingEnv/agents/kl-olop.json's settings on a StochasticMDP and a SparseMDP env of this package."""
    settings = {"__class__": OLOP_AGENT, "gamma": 0.8, "budget": 100, "upper_bound": {"type": "kullback-leibler", "c": 2},
                "lazy_tree_construction": True, "continuation_type": "uniform"}
    for cfg in (generators.random_stochastic(12, 3, seed=3), generators.random_sparse(12, 3, 2, seed=4)):
        env = env_of(cfg, 0)
        env.seed(5)
        agent = agent_factory(env, dict(settings))
        agent.seed(6)
        rng0 = native.rng_state_from_generator(agent.planner.np_random)
        pc = agent.planner.config
        thr = olr.thresholds(pc["upper_bound"]["threshold"], pc["upper_bound"]["time"], pc["episodes"])
        for _ in range(3):
            s0 = env.mdp.state
            res, rng0 = restated(cfg, s0, pc["episodes"], pc["horizon"], pc["gamma"], True, thr, "uniform", rng0)
            action = agent.act(s0)
            assert action == int(res["plan"][0])
            assert np.array_equal(native.rng_state_from_generator(agent.planner.np_random), rng0)
            env.step(action)
