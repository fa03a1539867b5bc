"""Robust OPD with one SET of M models per root: mp_model_load_joint_batch / mp_model_update_joint_tables /
mp_model_set_available_joint_batch and mp_ropd_plan_models, against mp_ropd_plan on each set loaded alone and against the CPU
oracle (which tests/test_per_episode_robust_host.py checks against the unmodified reference).  Everything is compared on bits:
the kernels are mp_ropd_plan's, only the states are global (set * S + local)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from rl_agents_amd import native
from rl_agents_amd.envs import generators
from tests.helpers import assert_form, opd_form
from tests.test_gpu_forms_reached import FORMS, KNOBS

pytestmark = pytest.mark.gpu

S, A, N = 12, 3, 5
MODEL_INDEX = np.array([0, 4, 2, 2, 1, 3, 0], np.int32)
BUDGET, GAMMA, TR = 60, 0.85, 0.25
MPL, CAP = BUDGET // A + 2, 1 + (BUDGET // A) * A


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def records(g, n):
    r = g.integers(0, 2 ** 63, size=(n, 6), dtype=np.int64).astype(np.uint64)
    r[:, 3] |= np.uint64(1)
    r[:, 4:] = 0
    return r


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def garnet_sets(n, m, seed, n_states=S, n_actions=A):
    """(t [n,m,S,A], r, term [n,m,S]): n * m independent garnets."""
    tabs = [[generators.random_deterministic(n_states, n_actions, seed=seed + 10 * b + k, terminal_rate=0.2) for k in range(m)]
            for b in range(n)]
    return (np.asarray([[c["transition"] for c in row] for row in tabs], np.int64),
            np.asarray([[c["reward"] for c in row] for row in tabs], np.float64),
            np.asarray([[c["terminal"] for c in row] for row in tabs]).astype(np.uint8))


def oracle_roots(t, r, term, mi, rs, rng, budget=BUDGET, gamma=GAMMA, tr=TR, mpl=MPL, done_rule="source", available=None):
    """The oracle on each root's own set, alone."""
    return [oracle.ropd_plan(t[b], r[b], term[b], rs[i], budget, gamma, tr, rng_state=rng[i].copy(), done_rule=done_rule,
                             max_plan_len=mpl, available=None if available is None else available[b])
            for i, b in enumerate(mi)]


def assert_equals_oracle(out, rng_after, refs, mpl=MPL):
    for i, ref in enumerate(refs):
        assert int(out["status"][i]) == native.MP_OK, i
        n = int(out["plan_len"][i])
        assert n == min(len(ref["plan"]), mpl) and out["plans"][i, :n].tolist() == ref["plan"][:n].tolist(), i
        assert bits(out["root_lower"][i]) == bits(ref["root_lower"]) and bits(out["root_upper"][i]) == bits(ref["root_upper"]), i
        assert int(out["env_steps"][i]) == ref["env_steps"], i
        np.testing.assert_array_equal(rng_after[i], ref["rng_after"], err_msg=str(i))


def assert_same_result(a, b):
    for k in ("status", "plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert np.array_equal(bits(a["root_lower"]), bits(b["root_lower"])) and np.array_equal(bits(a["root_upper"]), bits(b["root_upper"]))


# ---- 1. the batch against standalone models ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_batch_equals_each_set_loaded_alone_and_the_oracle(ctx, m):
    t, r, term = garnet_sets(N, m, seed=100 * m)
    model = ctx.load_joint_batch(t, r, term)
    assert (model.n_models, model.M, model.S_each, model.S, model.A) == (N, m, S, N * S, A)
    n_sets, s_each = C.c_int32(), C.c_int32()
    info = [C.c_int32() for _ in range(5)]
    assert ctx._lib.mp_model_batch_info(model._h, C.byref(n_sets), C.byref(s_each)) == 0
    assert ctx._lib.mp_model_info(model._h, *[C.byref(x) for x in info]) == 0
    assert (n_sets.value, s_each.value, info[1].value, info[2].value, info[3].value) == (N, S, m, N * S, A)
    g = np.random.Generator(np.random.PCG64(m))
    rs = g.integers(0, S, size=(len(MODEL_INDEX), m)).astype(np.int32)        # a joint state: every model in its own state
    rng0 = records(g, len(MODEL_INDEX))
    rng = rng0.copy()
    out = ctx.ropd_plan(model, rs, BUDGET, GAMMA, TR, rng, max_plan_len=MPL, model_index=MODEL_INDEX)
    form = opd_form(ctx, A, BUDGET, len(MODEL_INDEX), models=m)
    assert {1: "_m2", 2: "_m2", 3: "_m4", 5: "_gen"}[m] in form    # the m2, m4 and generic loops
    assert_form(ctx, form)
    refs = oracle_roots(t, r, term, MODEL_INDEX, rs, rng0)
    assert_equals_oracle(out, rng, refs)
    for root in (1, 3):                                 # the whole tree, states local to the root's set
        tree = ctx.ropd_tree(root, CAP, m)
        base = int(MODEL_INDEX[root]) * S
        assert ((tree["state"] >= base) & (tree["state"] < base + S)).all()
        tree["state"] = tree["state"] - base
        for k, want in refs[root]["tree"].items():
            np.testing.assert_array_equal(tree[k], want, err_msg="tree[{}] of root {}".format(k, root))
    # global joint states in mp_ropd_plan give the same
    rng_g = rng0.copy()
    assert_same_result(out, ctx.ropd_plan(model, rs + MODEL_INDEX[:, None] * S, BUDGET, GAMMA, TR, rng_g, max_plan_len=MPL))
    np.testing.assert_array_equal(rng_g, rng)
    for i, b in enumerate(MODEL_INDEX):                 # mp_ropd_plan on the root's set loaded alone
        alone = ctx.load_joint(t[b], r[b], term[b])
        rng_1 = rng0[i:i + 1].copy()
        one = ctx.ropd_plan(alone, rs[i:i + 1], BUDGET, GAMMA, TR, rng_1, max_plan_len=MPL)
        assert_same_result(one, {k: v[i:i + 1] for k, v in out.items()})
        np.testing.assert_array_equal(rng_1[0], rng[i])
        alone.close()
    model.close()


def test_export_tree_of_the_planner_reports_local_states(ctx):
    from rl_agents_amd.agents.robust.robust import DiscreteRobustPlanner
    t, r, term = garnet_sets(N, 2, seed=31)
    planner = DiscreteRobustPlanner(None, dict(budget=BUDGET, gamma=GAMMA, terminal_reward=TR))
    model = planner.models.ctx.load_joint_batch(t, r, term)
    g = np.random.Generator(np.random.PCG64(5))
    rs = g.integers(0, S, size=(len(MODEL_INDEX), 2)).astype(np.int32)
    rng0 = records(g, len(MODEL_INDEX))
    out = planner.plan_batch(None, rs, rng_states=rng0.copy(), model=model, model_index=MODEL_INDEX)
    ref = oracle_roots(t, r, term, MODEL_INDEX, rs, rng0, mpl=BUDGET // A + 1)[4]
    assert out["plans"][4, :out["plan_len"][4]].tolist() == ref["plan"].tolist()
    root = planner.export_tree(4)
    assert root.observation == tuple(int(s) for s in rs[4])
    nodes, k = [root], 0
    while k < len(nodes):
        nodes.extend(nodes[k].children.values())
        k += 1
    assert len(nodes) == len(ref["tree"]["parent"]) and all(0 <= s < S for n in nodes for s in n.observation)
    assert sorted(n.observation for n in nodes) == sorted(tuple(int(s) for s in row) for row in ref["tree"]["state"])
    model.close()


# ---- 2. every form family on a batch model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ropd_lds_m2", "ropd_lds_m4", "ropd_lds_gen", "ropd_lds_m2_chain", "ropd_wide_sib", "ropd_any"])
def test_every_form_family_on_a_batch_model(ctx, monkeypatch, name):
    case = FORMS[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in case["knobs"].split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv(k, v)
    a, budget, n, m, tr = case["n_actions"], case["budget"], case["n_roots"], case["models"], case["terminal_reward"]
    n_sets, n_states = 3, 60
    tabs = []
    for b in range(n_sets):
        cfg = generators.random_deterministic(n_states, a, seed=500 + a + 7 * b, terminal_rate=0.05)
        tabs.append([cfg] + [generators.rewire(cfg, 0.15, seed=10 + i + 5 * b) for i in range(m - 1)])
    t = np.asarray([[c["transition"] for c in row] for row in tabs], np.int64)
    r = np.asarray([[c["reward"] for c in row] for row in tabs], np.float64)
    term = np.asarray([[c["terminal"] for c in row] for row in tabs]).astype(np.uint8)
    g = np.random.Generator(np.random.PCG64(budget))
    mi = (np.arange(n) % n_sets).astype(np.int32)
    rs = np.repeat(g.integers(0, n_states, size=n).astype(np.int32)[:, None], m, axis=1)
    rng0 = records(g, n)
    rng = rng0.copy()
    mpl = budget // a + 2
    model = ctx.load_joint_batch(t, r, term)
    out = ctx.ropd_plan(model, rs, budget, 0.9, tr, rng, max_plan_len=mpl, model_index=mi)
    assert_form(ctx, name)
    for b in range(n_sets):
        sel = np.flatnonzero(mi == b)
        ref = oracle.ropd_plan_batch(t[b], r[b], term[b], rs[sel], budget, 0.9, tr, rng0[sel].copy(), max_plan_len=mpl)
        assert_same_result({k: v[sel] for k, v in out.items()}, ref)
        np.testing.assert_array_equal(rng[sel], ref["rng_after"])
    assert (out["status"] == 0).all()
    model.close()


# ---- 3. updates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("done_rule", ["source", "next"])
def test_updates_replace_whole_sets_and_keep_availability(ctx, done_rule):
    m = 2
    t, r, term = garnet_sets(N, m, seed=700)
    t2, r2, term2 = garnet_sets(N, m, seed=900)
    avail = np.asarray([[generators.random_available(S, A, seed=40 + 3 * b + k, rate=0.35) for k in range(m)] for b in range(N)])
    model = ctx.load_joint_batch(t, r, term, done_rule=done_rule, available=avail)
    g = np.random.Generator(np.random.PCG64(3))
    mi = np.array([0, 1, 2, 3, 4, 4, 2, 1, 0, 3], np.int32)
    rs = g.integers(0, S, size=(len(mi), m)).astype(np.int32)
    rng0 = records(g, len(mi))

    def plan(mdl):
        rng = rng0.copy()
        return ctx.ropd_plan(mdl, rs, BUDGET, GAMMA, TR, rng, max_plan_len=MPL, model_index=mi), rng
    before, rng_before = plan(model)
    assert_equals_oracle(before, rng_before, oracle_roots(t, r, term, mi, rs, rng0, done_rule=done_rule, available=avail))
    new_t, new_r, new_term = t.copy(), r.copy(), term.copy()
    for b in (1, 2, 4):
        new_t[b], new_r[b], new_term[b] = t2[b], r2[b], term2[b]
    model.update_tables(1, new_t[1:3], new_r[1:3], new_term[1:3])         # sets 1-2 in one call
    model.update_tables(4, new_t[4:5], new_r[4:5], new_term[4:5])         # set 4 in another
    after, rng_after = plan(model)
    fresh = ctx.load_joint_batch(new_t, new_r, new_term, done_rule=done_rule, available=avail)
    want, rng_want = plan(fresh)
    fresh.close()
    assert_same_result(after, want)
    np.testing.assert_array_equal(rng_after, rng_want)
    # the availability set before the update still holds: the oracle with the masks on the NEW tables
    assert_equals_oracle(after, rng_after, oracle_roots(new_t, new_r, new_term, mi, rs, rng0, done_rule=done_rule, available=avail))
    untouched = np.flatnonzero(np.isin(mi, (0, 3)))
    assert_same_result({k: v[untouched] for k, v in after.items()}, {k: v[untouched] for k, v in before.items()})
    touched = np.flatnonzero(np.isin(mi, (1, 2, 4)))
    assert any(after["plans"][i].tolist() != before["plans"][i].tolist() or after["root_lower"][i] != before["root_lower"][i]
               for i in touched)
    # a next state of S: MP_ERR_ARG, and the model is what it was
    bad = new_t[2:4].copy()
    bad[1, 1, 5, 2] = S
    with pytest.raises(native.NativeError) as err:
        model.update_tables(2, bad, r2[2:4], term2[2:4])
    assert err.value.code == native.MP_ERR_ARG
    with pytest.raises(native.NativeError) as err:
        model.update_tables(4, new_t[3:5], new_r[3:5], new_term[3:5])     # sets [4, 6) of 5
    assert err.value.code == native.MP_ERR_ARG
    again, rng_again = plan(model)
    assert_same_result(again, after)
    np.testing.assert_array_equal(rng_again, rng_after)
    model.close()


# ---- 4. availability ------------------------------------------------------------------------------------------------------------
def test_available_actions_are_the_union_over_a_sets_models(ctx):
    m = 2
    t, r, term = garnet_sets(N, m, seed=1300)
    avail = np.asarray([[generators.random_available(S, A, seed=80 + 3 * b + k, rate=0.45) for k in range(m)] for b in range(N)])
    union = avail.any(axis=1)
    # the union differs from each model's own mask somewhere, and some joint state lacks an action altogether
    assert (union != avail[:, 0]).any() and (union != avail[:, 1]).any() and not union.all()
    model = ctx.load_joint_batch(t, r, term)
    model.set_available(avail)
    g = np.random.Generator(np.random.PCG64(11))
    mi = np.arange(10, dtype=np.int32) % N
    rs = g.integers(0, S, size=(len(mi), m)).astype(np.int32)
    rng0 = records(g, len(mi))
    rng = rng0.copy()
    out = ctx.ropd_plan(model, rs, BUDGET, GAMMA, TR, rng, max_plan_len=MPL, model_index=mi)
    refs = oracle_roots(t, r, term, mi, rs, rng0, available=avail)
    assert_equals_oracle(out, rng, refs)
    plain = oracle_roots(t, r, term, mi, rs, rng0)
    assert any(int(out["env_steps"][i]) != plain[i]["env_steps"] for i in range(len(mi)))       # the masks do restrict something
    for root in (0, 7):
        tree = ctx.ropd_tree(root, CAP, m)
        tree["state"] = tree["state"] - int(mi[root]) * S
        for k, want in refs[root]["tree"].items():
            np.testing.assert_array_equal(tree[k], want, err_msg="tree[{}] of root {}".format(k, root))
        # the root's children: the union of what the two models list in their own root states (robust.py:22-25)
        b = int(mi[root])
        listed = np.flatnonzero(avail[b, 0, rs[root, 0]] | avail[b, 1, rs[root, 1]])
        first, count = int(tree["first_child"][0]), int(tree["n_children"][0])
        assert tree["action"][first:first + count].tolist() == listed.tolist()
    with pytest.raises(native.NativeError) as err:      # a (set, model, state) without any action
        none = avail.copy()
        none[3, 1, 4] = False
        model.set_available(none)
    assert err.value.code == native.MP_ERR_ARG
    model.close()


# ---- 5. device-resident arrays --------------------------------------------------------------------------------------------------
def test_device_arrays_and_device_generators_give_the_host_results(ctx):
    import torch
    m = 3
    t, r, term = garnet_sets(N, m, seed=1700)
    model = ctx.load_joint_batch(t, r, term)
    g = np.random.Generator(np.random.PCG64(17))
    n = 70
    mi = g.integers(0, N, size=n).astype(np.int32)
    rs = g.integers(0, S, size=(n, m)).astype(np.int32)
    rng0 = records(g, n)
    rng = rng0.copy()
    host = ctx.ropd_plan(model, rs, BUDGET, GAMMA, TR, rng, max_plan_len=MPL, model_index=mi)
    # MP_MEM_DEVICE: every array a device tensor
    dev = torch.device("cuda", ctx.device)
    d = dict(mi=torch.from_numpy(mi).to(dev), rs=torch.from_numpy(rs).to(dev), rng=torch.from_numpy(rng0.view(np.int64)).to(dev),
             plans=torch.full((n, MPL), -1, dtype=torch.int32, device=dev), plan_len=torch.zeros(n, dtype=torch.int32, device=dev),
             lower=torch.zeros(n, dtype=torch.float64, device=dev), upper=torch.zeros(n, dtype=torch.float64, device=dev),
             steps=torch.zeros(n, dtype=torch.int64, device=dev), status=torch.zeros(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ctx.ropd_plan_device(model, n, d["rs"], BUDGET, GAMMA, TR, d["rng"], MPL, plans=d["plans"], plan_len=d["plan_len"],
                         root_lower=d["lower"], root_upper=d["upper"], env_steps=d["steps"], status=d["status"], model_index=d["mi"])
    ctx.synchronize()
    assert ctx.device_faults() == 0
    got = dict(status=d["status"].cpu().numpy(), plans=d["plans"].cpu().numpy(), plan_len=d["plan_len"].cpu().numpy(),
               env_steps=d["steps"].cpu().numpy(), root_lower=d["lower"].cpu().numpy(), root_upper=d["upper"].cpu().numpy())
    assert_same_result(got, host)
    np.testing.assert_array_equal(d["rng"].cpu().numpy().view(np.uint64), rng)
    # MP_MEM_RNG_DEVICE: host arrays, the generator records resident on the device
    dev_rng = ctx.device_rng(rng0)
    out = dict(plans=np.full((n, MPL), -1, np.int32), plan_len=np.zeros(n, np.int32), root_lower=np.zeros(n), root_upper=np.zeros(n),
               env_steps=np.zeros(n, np.int64), status=np.zeros(n, np.int32))
    rc = ctx._lib.mp_ropd_plan_models(ctx._h, model._h, n, mi.ctypes.data, rs.ctypes.data, BUDGET, GAMMA, TR, dev_rng.ptr(0), MPL,
                                      out["plans"].ctypes.data, out["plan_len"].ctypes.data, out["root_lower"].ctypes.data,
                                      out["root_upper"].ctypes.data, out["env_steps"].ctypes.data, out["status"].ctypes.data,
                                      native.MP_MEM_HOST | native.MP_MEM_RNG_DEVICE)
    assert rc == native.MP_OK
    assert_same_result(out, host)
    np.testing.assert_array_equal(dev_rng.get(), rng)
    dev_rng.close()
    # device arrays cannot be validated on the host: a bad set or local state is clamped to state 0 of set 0 and counted
    bad_mi, bad_rs = mi.copy(), rs.copy()
    bad_mi[5], bad_rs[9, 1], bad_rs[20, 2] = N, S, -1
    d["mi"].copy_(torch.from_numpy(bad_mi))
    d["rs"].copy_(torch.from_numpy(bad_rs))
    d["rng"].copy_(torch.from_numpy(rng0.view(np.int64)))
    torch.cuda.synchronize()
    ctx.ropd_plan_device(model, n, d["rs"], BUDGET, GAMMA, TR, d["rng"], MPL, plans=d["plans"], plan_len=d["plan_len"],
                         root_lower=d["lower"], root_upper=d["upper"], env_steps=d["steps"], status=d["status"], model_index=d["mi"])
    torch.cuda.synchronize()
    assert ctx.device_faults() == 3
    with pytest.raises(native.NativeError, match="out of range"):
        ctx.synchronize()
    ctx.synchronize()                                   # reported once
    clamped = oracle.ropd_plan(t[0], r[0], term[0], np.zeros(m, np.int32), BUDGET, GAMMA, TR, rng_state=rng0[9].copy(), max_plan_len=MPL)
    plans = d["plans"].cpu().numpy()
    assert plans[9, :int(d["plan_len"][9])].tolist() == clamped["plan"].tolist()
    good = np.setdiff1d(np.arange(n), [5, 9, 20])
    np.testing.assert_array_equal(plans[good], host["plans"][good])
    model.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    m = 2
    t, r, term = garnet_sets(N, m, seed=2100)
    model = ctx.load_joint_batch(t, r, term)
    g = np.random.Generator(np.random.PCG64(23))
    mi = MODEL_INDEX.copy()
    rs = g.integers(0, S, size=(len(mi), m)).astype(np.int32)
    rng0 = records(g, len(mi))

    def code(call):
        with pytest.raises(native.NativeError) as err:
            call()
        return err.value.code
    # host arrays out of range
    for bad_mi, bad_rs in ((np.where(np.arange(len(mi)) == 2, N, mi), rs), (np.where(np.arange(len(mi)) == 2, -1, mi), rs),
                           (mi, np.where(np.arange(rs.size).reshape(rs.shape) == 5, S, rs)),
                           (mi, np.where(np.arange(rs.size).reshape(rs.shape) == 5, -1, rs))):
        assert code(lambda: ctx.ropd_plan(model, bad_rs.astype(np.int32), BUDGET, GAMMA, TR, rng0.copy(), max_plan_len=MPL,
                                          model_index=bad_mi.astype(np.int32))) == native.MP_ERR_ARG
    # anything but a joint batch model
    plain_joint = ctx.load_joint(t[0], r[0], term[0])
    table_batch = ctx.load_table_batch(t[:, 0], r[:, 0], term[:, 0])
    dense_cfg = generators.random_stochastic(S, A, seed=1)
    dense = ctx.load_dense(dense_cfg["transition"], dense_cfg["reward"], dense_cfg["terminal"])
    sparse_cfg = generators.random_sparse(S, A, 2, seed=1)
    sparse = ctx.load_sparse(sparse_cfg["transition"], sparse_cfg["next"], sparse_cfg["reward"], sparse_cfg["terminal"])
    zeros = np.zeros(len(mi), np.int32)
    for other in (plain_joint, table_batch, dense, sparse):
        other.M = m                                      # (only shapes the root_state array on the Python side)
        assert code(lambda: ctx.ropd_plan(other, rs, BUDGET, GAMMA, TR, rng0.copy(), max_plan_len=MPL, model_index=zeros)) == native.MP_ERR_MODE
        other.close()
    # the table-batch update entry points go on refusing every joint model
    assert ctx._lib.mp_model_update_tables(model._h, 0, 1, t[0, 0].ctypes.data, r[0, 0].ctypes.data, term[0, 0].ctypes.data) == native.MP_ERR_MODE
    rows = np.zeros(1, np.int32)
    assert ctx._lib.mp_model_update_rows(model._h, 1, rows.ctypes.data, t[0, 0, :1].ctypes.data, r[0, 0, :1].ctypes.data, None) == native.MP_ERR_MODE
    # ... and the single-table availability calls (their flags would not survive an update of the sets)
    assert code(lambda: native.Model.set_available(model, np.ones((N * S, A), bool))) == native.MP_ERR_MODE
    ones = np.ones((m, N * S, A), np.uint8)
    assert ctx._lib.mp_model_set_available_joint(model._h, ones.ctypes.data) == native.MP_ERR_MODE
    # a shape whose global records do not fit 31 bits: refused before anything is allocated
    h = C.c_void_p()
    assert ctx._lib.mp_model_load_joint_batch(ctx._h, 1 << 20, 2, 1 << 10, 4, t.ctypes.data, r.ctypes.data, None, 0, C.byref(h)) == native.MP_ERR_ARG
    assert "31 bits" in native.load().mp_last_error().decode()
    # ... and one whose N * M * S * A records are beyond the device's memory (2^36 of them)
    assert ctx._lib.mp_model_load_joint_batch(ctx._h, 1 << 18, 64, 1 << 10, 4, t.ctypes.data, r.ctypes.data, None, 0, C.byref(h)) == native.MP_ERR_ARG
    assert "exceed the device's" in native.load().mp_last_error().decode()
    # one set with a reward of 1.5: MP_ERR_REWARD_RANGE for its roots only
    r_bad = r.copy()
    r_bad[2, 1] = 1.5
    model.update_tables(2, t[2:3], r_bad[2:3], term[2:3])
    rng = rng0.copy()
    out = ctx.ropd_plan(model, rs, BUDGET, GAMMA, TR, rng, max_plan_len=MPL, model_index=mi)
    on_bad = mi == 2
    assert on_bad.sum() == 2 and (out["status"][on_bad] == native.ERR_REWARD_RANGE).all() and (out["status"][~on_bad] == native.MP_OK).all()
    good = np.flatnonzero(~on_bad)
    refs = oracle_roots(t, r, term, mi[good], rs[good], rng0[good])
    assert_equals_oracle({k: v[good] for k, v in out.items()}, rng[good], refs)
    model.close()
