"""Sparse Sampling on a batch model with one MDP per root (mp_ss_plan_models, the kernel forms of mp_ss_each_form_names)
against the test-side restatement (tests/sparse_sampling_restatement.py) run on each root's OWN table alone.

Everything on bits: plans, root values, samples, the generator records after the plan and every array of the exported trees,
whose decision keys are GLOBAL states, model_index * S_each + local.  The last test plans the steps of the unmodified reference's
per-episode agents (tests/golden/per_episode_sparse_sampling.npz) through the entry point."""
import os

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.envs import generators
from tests import sparse_sampling_restatement as sr
from tests.helpers import assert_form, generator_from

pytestmark = pytest.mark.gpu

FORMS = [name[len("ss_each_"):] for name in native.ss_each_form_names()]
GAMMA = 0.8


@pytest.fixture(scope="module")
def ctx():
    return native.Context(0)


def stack(tabs):
    return (np.stack([t["transition"] for t in tabs]).astype(np.int64), np.stack([t["reward"] for t in tabs]).astype(np.float64),
            np.stack([np.asarray(t["terminal"]) for t in tabs]).astype(np.uint8))


def load(ctx, tabs, available=None, order=None):
    """The batch model of `tabs`; with a listing order the device's columns are the env's actions in that order."""
    t, r, term = stack(tabs)
    if order is not None:
        t, r = t[:, :, order], r[:, :, order]
    model = ctx.load_table_batch(t, r, term)
    if available is not None:
        av = np.stack(available)
        model.set_available(av[:, :, order].reshape(-1, av.shape[2]) if order is not None else av.reshape(-1, av.shape[2]))
    return model


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def restated(tab, s0, horizon, n_samples, rng6, available=None, order=None):
    """The restatement on ONE table from LOCAL state s0 -> (result, generator record after)."""
    gen = generator_from(rng6)
    res = sr.ss_plan("deterministic", tab["transition"], tab["reward"], int(s0), horizon, n_samples, GAMMA, gen, available=available,
                     order=order)
    return res, native.rng_state_from_generator(gen)


def assert_root(out, rng, i, res, rng_after, order=None):
    assert res["error"] is None and int(out["status"][i]) == native.MP_OK, i
    plan = int(out["plans"][i])
    assert [plan if order is None else int(order[plan])] == res["plan"].tolist(), i
    assert bits(out["root_value"][i]) == bits(res["root_value"]), i
    assert int(out["samples"][i]) == res["samples"], i
    assert np.array_equal(rng[i], rng_after), i


def assert_tree(tree, res, base, order=None):
    """A whole exported tree == the restatement's, its states moved to the MDP's block of GLOBAL states and its actions, which
    the device labels by column, back to the environment's ids."""
    chance = np.asarray(res["is_chance"]).astype(bool)
    key = np.where(~chance & (np.asarray(res["parent"]) >= 0), np.asarray(res["key"]) + base, res["key"])
    got = tree["key"] if order is None else np.where(tree["is_chance"].astype(bool), np.asarray(order)[np.where(chance, tree["key"], 0)],
                                                      tree["key"])
    for k in ("parent", "is_chance", "depth", "count"):
        assert np.array_equal(tree[k], res[k]), k
    assert np.array_equal(got, key), "key"
    assert np.array_equal(bits(tree["value"]), bits(res["value"])), "value"


def check(ctx, tabs, model, model_index, local, horizon, n_samples, sample, form, tree_roots=(), available=None, order=None, seed=11):
    n, s_each = len(model_index), tabs[0]["reward"].shape[0]
    rng = native.seed_sequence_states([seed], 0, n)
    rng0 = rng.copy()
    out = ctx.ss_plan(model, np.asarray(local, np.int32), horizon, n_samples, GAMMA, rng, model_index=np.asarray(model_index, np.int32))
    assert_form(ctx, "ss_each_" + form)
    for i in sample:
        m = int(model_index[i])
        res, rng_after = restated(tabs[m], local[i], horizon, n_samples, rng0[i], None if available is None else available[m], order)
        assert_root(out, rng, i, res, rng_after, order)
        if i in tree_roots:
            assert_tree(ctx.ss_tree(i), res, m * s_each, order)
    return out, rng0, rng


# ------------------------------------------------------------------------------------------------------------ 1. own tables
SMALL = dict(model_index=[3, 0, 3, 1, 4, 0, 2], local=[0, 5, 2, 4, 1, 3, 5])      # tables 3 and 0 are shared by two roots each


@pytest.fixture(scope="module")
def small_tables():
    return [generators.random_deterministic(6, 2, seed=20 + k, terminal_rate=0.2) for k in range(5)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("horizon,n_samples", [(1, 1), (2, 2), (3, 2), (2, 65)])
def test_every_root_plans_on_its_own_table(ctx, monkeypatch, small_tables, horizon, n_samples, form):
    """(2, 65): with 2 actions the one-pass last level takes 130 samples, and an action's 65 samples straddle the 64-lane
    chunks."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    model = load(ctx, small_tables)
    check(ctx, small_tables, model, SMALL["model_index"], SMALL["local"], horizon, n_samples, range(7), form, tree_roots=range(7))
    model.close()


# --------------------------------------------------------------------------------------------------- 2. equal to mp_ss_plan
@pytest.mark.parametrize("form", FORMS)
def test_equal_to_the_plain_entry_point_on_one_table(ctx, monkeypatch, small_tables, form):
    monkeypatch.setenv("MP_EACH_MODEL", form)
    model = load(ctx, small_tables)
    rng = native.seed_sequence_states([11], 0, 7)
    rng0 = rng.copy()
    out = ctx.ss_plan(model, np.asarray(SMALL["local"], np.int32), 3, 2, GAMMA, rng, model_index=np.asarray(SMALL["model_index"], np.int32))
    assert_form(ctx, "ss_each_" + form)
    roots = [i for i, m in enumerate(SMALL["model_index"]) if m == 3]
    trees = {i: ctx.ss_tree(i) for i in roots}
    tab = small_tables[3]
    plain = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
    rng1 = np.ascontiguousarray(rng0[roots])
    ref = ctx.ss_plan(plain, np.asarray(SMALL["local"], np.int32)[roots], 3, 2, GAMMA, rng1)
    assert_form(ctx, "ss_wave_lds")
    for k in ("plans", "samples", "status"):
        assert np.array_equal(out[k][roots], ref[k]), k
    assert np.array_equal(bits(out["root_value"][roots]), bits(ref["root_value"]))
    assert np.array_equal(rng[roots], rng1)
    for j, i in enumerate(roots):
        want = ctx.ss_tree(j)
        decision = (want["is_chance"] == 0) & (want["parent"] >= 0)
        want["key"] = np.where(decision, want["key"] + 3 * 6, want["key"])
        for k in want:
            assert np.array_equal(trees[i][k].view(np.uint8), want[k].view(np.uint8)), (i, k)
    plain.close()
    model.close()


# ------------------------------------------------------------------------------------- 3. more roots than workgroups (stale LDS)
@pytest.mark.parametrize("form", FORMS)
def test_a_workgroup_reloads_the_table_of_its_next_root(ctx, monkeypatch, form):
    """Some workgroups plan two roots.  First run: the two own different tables -- a root served from the previous root's copy
    would plan on the wrong MDP.  Second run: they own the same table -- the copy is skipped."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    cus = ctx.device_info()["n_cu"]
    grid = native.each_form_info("ss", 6, 2, 2, 1 << 30, cus)["grid"]
    n = grid + 3
    info = native.each_form_info("ss", 6, 2, 2, n, cus)
    assert info["grid"] == grid and info["lds"] == (form == "lds")
    tabs = [generators.random_deterministic(6, 2, seed=100 + k, terminal_rate=0.1) for k in range(64)]
    model = load(ctx, tabs)
    roots = np.arange(n)
    local = (5 * roots + roots // 64) % 6
    always = {0, 1, 2, n - 3, n - 2, n - 1}                  # the three workgroups that take two roots, both of them
    sample = sorted(always | set(np.random.default_rng(5).choice(np.arange(3, n - 3), size=64, replace=False).tolist()))
    differ = (7 * roots + roots // grid) % 64
    assert all(differ[r] != differ[r + grid] for r in range(3))
    check(ctx, tabs, model, differ, local, 2, 2, sample, form, tree_roots=(0, n - 3, n - 1))
    equal = (7 * (roots % grid)) % 64
    assert all(equal[r] == equal[r + grid] for r in range(3))
    check(ctx, tabs, model, equal, local, 2, 2, sample, form, tree_roots=(0, n - 3, n - 1))
    model.close()


# ------------------------------------------------------------------------------------- 4. restricted and re-ordered actions
@pytest.mark.parametrize("form", FORMS)
def test_restricted_and_reordered_actions(ctx, monkeypatch, form):
    monkeypatch.setenv("MP_EACH_MODEL", form)
    S, A = 8, 4
    tabs = [generators.random_deterministic(S, A, seed=200 + k, terminal_rate=0.1) for k in range(3)]
    avail = [generators.random_available(S, A, seed=210 + k, rate=0.4) for k in range(3)]
    avail[1][5] = [False, False, True, False]                # the state of root 2: a single listed action, no tie draw
    avail[0][int(tabs[0]["transition"][2, 1])] = [False, True, False, False]   # a state below root 0 that lists a single action
    avail[0][2, 1] = True
    order = [2, 0, 3, 1]
    model = load(ctx, tabs, avail, order)
    model_index, local = [0, 2, 1, 1, 0], [2, 7, 5, 0, 6]
    out, rng0, rng = check(ctx, tabs, model, model_index, local, 3, 2, range(5), form, tree_roots=range(5), available=avail, order=order)
    assert int(np.asarray(order)[out["plans"][2]]) == 2
    assert out["samples"][2] < out["samples"].max()
    model.close()


# -------------------------------------------------------------------------------------------------------------- 5. root ties
@pytest.mark.parametrize("form", FORMS)
def test_root_ties_are_drawn(ctx, monkeypatch, form):
    """Equal rewards everywhere: every root's chance children tie, random_argmax draws among them (abstract.py:296-311) after the
    samples' draws; the generator record after the plan and the chosen action are the restatement's."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    tabs = []
    for k in range(3):
        tab = generators.random_deterministic(6, 3, seed=300 + k)
        tab["reward"] = np.full((6, 3), 0.5)
        tabs.append(tab)
    model = load(ctx, tabs)
    model_index, local = np.arange(12) % 3, np.arange(12) % 6
    out, rng0, rng = check(ctx, tabs, model, model_index, local, 2, 3, range(12), form, tree_roots=(0, 11))
    assert len(set(out["plans"].tolist())) > 1               # (twelve draws among three: not all the first maximum)
    # 3 + 9 samples of one 32-bit draw each, then the tie draw: not the record twelve draws alone leave
    gen = generator_from(rng0[0])
    gen.integers(2 ** 30, size=12)
    assert not np.array_equal(native.rng_state_from_generator(gen), rng[0])
    model.close()


# ------------------------------------------------------------------------------------------------------ 6. the LDS boundary
@pytest.mark.parametrize("form", FORMS)
def test_the_largest_table_in_lds_and_the_next_one(ctx, monkeypatch, form):
    """MP_EACH_MODEL=lds: the largest S_each at |A| = 3 that fits a compute unit's LDS behind the frames -- a launch with more than
    64 KiB of dynamic LDS -- and the next one, where the knob is ignored."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    cus = ctx.device_info()["n_cu"]
    info = native.each_form_info("ss", 1, 3, 1, 1, cus)
    s_max = (info["fit_limit"] - 64) // 48
    for s_each, taken in ((s_max, form), (s_max + 1, "global")):
        assert native.each_form_info("ss", s_each, 3, 1, 1, cus)["lds"] == (taken == "lds")
        tabs = [generators.random_deterministic(s_each, 3, seed=400, terminal_rate=0.05)]
        model = load(ctx, tabs)
        check(ctx, tabs, model, [0], [s_each - 1], 1, 2, range(1), taken, tree_roots=(0,))
        model.close()


# ------------------------------------------------------------------------------------------ 7. update_tables between two plans
@pytest.mark.parametrize("form", FORMS)
def test_update_tables_between_two_plans(ctx, monkeypatch, small_tables, form):
    monkeypatch.setenv("MP_EACH_MODEL", form)
    model = load(ctx, small_tables)
    first, rng0, _ = check(ctx, small_tables, model, SMALL["model_index"], SMALL["local"], 3, 2, range(7), form)
    new = list(small_tables)
    new[3] = generators.random_deterministic(6, 2, seed=99, terminal_rate=0.2)
    t, r, term = stack([new[3]])
    model.update_tables(3, t, r, term)
    second, rng1, _ = check(ctx, new, model, SMALL["model_index"], SMALL["local"], 3, 2, range(7), form)   # (same seeds)
    assert np.array_equal(rng0, rng1)
    others = [i for i, m in enumerate(SMALL["model_index"]) if m != 3]
    for k in ("plans", "samples", "status"):
        assert np.array_equal(first[k][others], second[k][others]), k
    assert np.array_equal(bits(first["root_value"][others]), bits(second["root_value"][others]))
    assert not np.array_equal(bits(first["root_value"]), bits(second["root_value"]))
    model.close()


# -------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(ctx, monkeypatch, small_tables):
    monkeypatch.delenv("MP_EACH_MODEL", raising=False)
    rng = native.seed_sequence_states([3], 0, 2)

    def code(model, model_index, local, horizon=2, n_samples=2):
        with pytest.raises(native.NativeError) as e:
            ctx.ss_plan(model, np.asarray(local, np.int32), horizon, n_samples, GAMMA, rng.copy(),
                        model_index=None if model_index is None else np.asarray(model_index, np.int32))
        return e.value.code

    dense = generators.random_stochastic(8, 2, seed=1)
    sparse = generators.random_sparse(8, 2, 2, seed=2)
    t, r, term = stack(small_tables[:2])
    others = [ctx.load_dense(dense["transition"], dense["reward"], dense["terminal"]),
              ctx.load_sparse(sparse["transition"], sparse["next"], sparse["reward"], sparse["terminal"]),
              ctx.load_joint(t, r, term)]
    for model in others:
        assert code(model, [0, 0], [1, 2]) == native.MP_ERR_MODE
        model.close()
    model = load(ctx, small_tables)
    assert code(model, [0, 1], [1, 2], horizon=17) == native.MP_ERR_ARG
    assert code(model, [0, 1], [1, 2], horizon=0) == native.MP_ERR_ARG
    assert code(model, [0, 1], [1, 2], n_samples=1025) == native.MP_ERR_ARG
    assert code(model, [0, 1], [1, 2], n_samples=0) == native.MP_ERR_ARG
    for bad in ([0, 5], [-1, 0]):                           # model_index outside [0, N) in a host array
        assert code(model, bad, [1, 2]) == native.MP_ERR_ARG
    assert code(model, [0, 1], [1, 6]) == native.MP_ERR_ARG  # a local state outside [0, S_each)
    assert code(model, None, [1, 2]) == native.MP_ERR_MODE   # mp_ss_plan itself keeps refusing batch models
    model.close()


# ------------------------------------------------------------------------- 9. the unmodified reference's per-episode agents
@pytest.mark.parametrize("form", FORMS)
def test_golden_per_episode_steps_through_the_entry_point(ctx, monkeypatch, form):
    """Seven episodes of the reference, each with its own agent object and a table replaced before every step, planned as a lock-
    step would plan them: update_tables, then ONE ss_plan(..., model_index=...) over the live episodes (the last episode ends
    early and drops out).  Every plan, every generator record before and after, every root value on bits."""
    monkeypatch.setenv("MP_EACH_MODEL", form)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "per_episode_sparse_sampling.npz"))
    n, steps = len(z["s0"]), z["transition"].shape[1]
    horizon, n_samples, gamma = int(z["ss/horizon"]), int(z["ss/C"]), float(z["ss/gamma"])
    n_steps = [int(z["ss/e{}/n_steps".format(e)]) for e in range(n)]
    assert min(n_steps) < steps == max(n_steps)
    rng = np.stack([z["ss/e{}/rng_before".format(e)] for e in range(n)])
    model, ties = None, 0
    for t in range(steps):
        tr, rw, term = z["transition"][:, t], z["reward"][:, t], z["terminal"][:, t].astype(np.uint8)
        if model is None:
            model = ctx.load_table_batch(tr, rw, term)
        else:
            model.update_tables(0, tr, rw, term)
        live = np.array([e for e in range(n) if t < n_steps[e]], np.int32)
        states = np.array([z["ss/e{}/states".format(e)][t] for e in live], np.int32)
        for e in live:
            np.testing.assert_array_equal(rng[e], z["ss/e{}/t{}/rng_before".format(e, t)])
        live_rng = np.ascontiguousarray(rng[live])
        out = ctx.ss_plan(model, states, horizon, n_samples, gamma, live_rng, model_index=live)
        assert_form(ctx, "ss_each_" + form)
        rng[live] = live_rng
        for k, e in enumerate(live):
            p = "ss/e{}/t{}".format(e, t)
            assert [int(out["plans"][k])] == z[p + "/plan"].tolist(), p
            np.testing.assert_array_equal(rng[e], z[p + "/rng_after"], err_msg=p)
            assert bits(out["root_value"][k]) == bits(z[p + "/root_value"]), p
            ties = max(ties, int(z[p + "/root_ties"]))
    assert ties >= 2                                 # the tie draw of random_argmax is among the recorded plans
    model.close()


# ------------------------------------------------------------------------------------------------------ 10. device arrays
def _device_call(ctx, model, model_index, local, rng, horizon, n_samples):
    """mp_ss_plan_models on device tensors (MP_MEM_DEVICE): the (model_index, local state) pairs become global states in one
    small launch, which clamps and counts what is out of range.  -> the tensors, still on the device."""
    import torch
    n = len(local)
    dev = torch.device("cuda", ctx.device)
    d = dict(mi=torch.from_numpy(np.asarray(model_index, np.int32)).to(dev), s0=torch.from_numpy(np.asarray(local, np.int32)).to(dev),
             rng=torch.from_numpy(rng.view(np.int64).copy()).to(dev), plans=torch.full((n,), -1, dtype=torch.int32, device=dev),
             value=torch.zeros(n, dtype=torch.float64, device=dev), samples=torch.zeros(n, dtype=torch.int64, device=dev),
             status=torch.full((n,), -1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ptr = native._ptr
    native._check(ctx._lib.mp_ss_plan_models(ctx._h, model._h, n, ptr(d["mi"]), ptr(d["s0"]), horizon, n_samples, GAMMA, ptr(d["rng"]),
                                             ptr(d["plans"]), ptr(d["value"]), ptr(d["samples"]), ptr(d["status"]),
                                             native.MP_MEM_DEVICE))
    return d


@pytest.mark.parametrize("form", FORMS)
def test_device_arrays_and_out_of_range_roots(ctx, monkeypatch, small_tables, form):
    """Device arrays cannot be validated on the host: as for mp_opd_plan_models a root naming a model / state out of range is
    clamped to state 0 of model 0 (nothing is read out of bounds), counted, and the next synchronize() raises once; every
    root's results are those of the pair it planned on."""
    import torch
    monkeypatch.setenv("MP_EACH_MODEL", form)
    model = load(ctx, small_tables)
    n = 16
    mi, s0 = (np.arange(n) % 5).astype(np.int32), (np.arange(n) * 5 % 6).astype(np.int32)
    rng0 = native.seed_sequence_states([21], 0, n)

    def compare(d, planned_mi, planned_s0):
        rng = d["rng"].cpu().numpy().view(np.uint64)
        out = dict(plans=d["plans"].cpu().numpy(), root_value=d["value"].cpu().numpy(), samples=d["samples"].cpu().numpy(),
                   status=d["status"].cpu().numpy())
        for i in range(n):
            res, rng_after = restated(small_tables[int(planned_mi[i])], planned_s0[i], 2, 3, rng0[i])
            assert_root(out, rng, i, res, rng_after)

    d = _device_call(ctx, model, mi, s0, rng0, 2, 3)
    ctx.synchronize()
    assert_form(ctx, "ss_each_" + form)
    assert ctx.device_faults() == 0
    compare(d, mi, s0)
    bad_mi, bad_s0 = mi.copy(), s0.copy()
    bad_mi[3], bad_mi[7], bad_s0[9], bad_s0[12] = 5, -1, 6, -2
    d = _device_call(ctx, model, bad_mi, bad_s0, rng0, 2, 3)
    torch.cuda.synchronize()
    assert ctx.device_faults() == 4
    with pytest.raises(native.NativeError, match="out of range"):
        ctx.synchronize()
    ctx.synchronize()                                   # reported once
    assert ctx.device_faults() == 0
    fixed_mi, fixed_s0 = mi.copy(), s0.copy()
    for i in (3, 7, 9, 12):
        fixed_mi[i], fixed_s0[i] = 0, 0                 # what the clamped roots planned on
    compare(d, fixed_mi, fixed_s0)
    model.close()
