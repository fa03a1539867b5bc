"""The two VI kernels whose workgroups wait for each other: the cluster form of mp_vi_solve_batch
(vi_det_batch_cluster<AT, OWN>: K = 2 / 4 / 8 workgroups per MDP) and the persistent single-MDP solver (vi_det_persist).

Every case is compared bit for bit with the CPU oracle (value_iteration.py:42-45,65-73 per MDP), on outputs that expose
memory nobody wrote: device tensors pre-filled with NaN, and host arrays after a call on other tables (a stale staging
buffer holds that call's Q).

  * every instantiation of the cluster form the dispatcher can reach (|A| = 2..6 x (K, OWN)) at the edges of its state
    slices, and the first shapes past it;
  * ONE workgroup of a cluster giving up while its partners carry on (MP_VI_BATCH_CLUSTER_GIVE_UP) -- at the MDP's last sweep
    the partners finish with real values, and only the MDP's give-up word sends it to the follow-up launch;
  * a NULL sweeps_out through the C ABI while clusters fail;
  * one workgroup of the persistent grid giving up (MP_VI_PERSIST_GIVE_UP)."""
import os

import numpy as np
import pytest

from rl_agents_amd import native
from tests.helpers import assert_form, assert_vi_batch_form

pytestmark = pytest.mark.gpu

K_LAG = 2                                   # vi.hip kLag: the persistent kernel reads a sweep's verdict kLag sweeps late


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def _cdiv(a, b):
    return -(-a // b)


def _geometry(S, K, A=5):
    """What the solve chooses for MDPs of S states under the knobs the cluster tests below set (native.vi_batch_geometry: the
    function the solve launches from; the forced K makes the batch size and the device's size irrelevant).  Also called while
    the module is collected, so the knobs are set here and put back."""
    knobs = dict(MP_VI_BATCH_NO_REG="1", MP_VI_BATCH_CLUSTER=str(K))
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        return native.vi_batch_geometry(3, S, A, 200)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def _takes_cluster(S, K, own=3):
    """S takes the cluster form at K workgroups per MDP, a thread keeping at most ``own`` states."""
    g = _geometry(S, K)
    return g["form"] == "cluster" and g["k"] == K and g["own"] <= own


def _last_cluster(K, own=3):
    """The largest S with _takes_cluster (it holds up to some S and never after), 0 if there is none."""
    lo, hi = 0, 1 << 16
    assert not _takes_cluster(hi, K, own)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _takes_cluster(mid, K, own) else (lo, mid)
    return lo


def _reachable():
    """(K, OWN) pairs the dispatcher can reach: OWN 1..3 at K = 2 and 4, 1..2 at K = 8 (LDS)."""
    return [(K, own) for K in (2, 4, 8) for own in (1, 2, 3) if _last_cluster(K, own) > _last_cluster(K, own - 1)]


def _edges(K, own):
    """S at the edges of the slices of (K, OWN): the first S of OWN, the last one where every slice is full (the LDS may end the
    form before that), a ragged last slice (S = 1 mod K), and at OWN = 1 a shape whose last parts own no state."""
    lo, hi = _last_cluster(K, own - 1) + 1, _last_cluster(K, own)
    out = [lo]
    if hi == K * _geometry(hi, K)["block"] * own:
        out.append(hi)
    out.append(hi - (hi - 1) % K)
    if own == 1:
        out.append(K + 1 if K > 2 else 1)
    return sorted(set(out))


def _tables(n, S, A, seed, terminal=True, scales=None):
    """Random deterministic tables (free |A| and S); per-MDP reward scales make the MDPs of one launch stop at different
    sweeps (small rewards pass allclose's atol sooner)."""
    g = np.random.default_rng(seed)
    tr = g.integers(0, S, size=(n, S, A), dtype=np.int64)
    rw = g.random((n, S, A))
    if scales is None:
        scales = 10.0 ** -(3 * (np.arange(n) % 4))
    rw *= np.asarray(scales, np.float64)[:, None, None]
    tm = (g.random((n, S)) < 0.1).astype(np.uint8) if terminal else None
    return tr, rw, tm


def _nan_outputs(n, S, A):
    import torch
    dq = torch.full((n * S, A), float("nan"), dtype=torch.float64, device="cuda")
    dsw = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                # (filled on torch's stream; the library enqueues on its own)
    return dq, dsw


def _check_device(ctx, model, gamma, iters, ref, variant):
    n, S, A = ref[0].shape
    dq, dsw = _nan_outputs(n, S, A)
    ctx.vi_solve_batch_device(model, gamma, iters, dq, dsw)
    ctx.synchronize()
    assert ctx.last_kernel_variant() == variant
    assert_vi_batch_form(ctx, n, S, A, iters)
    np.testing.assert_array_equal(dsw.cpu().numpy(), ref[1])
    q = dq.cpu().numpy().reshape(n, S, A)
    assert np.array_equal(q, ref[0]), "device Q differs in MDPs {}".format(
        sorted({int(b) for b in np.argwhere(~(q == ref[0]))[:, 0]}))


def _check_host(ctx, model, gamma, iters, ref, variant):
    q, sw = ctx.vi_solve_batch(model, gamma, iters)
    assert ctx.last_kernel_variant() == variant
    assert_vi_batch_form(ctx, *ref[0].shape, iters)
    np.testing.assert_array_equal(sw, ref[1])
    assert np.array_equal(q, ref[0]), "host Q differs in MDPs {}".format(
        sorted({int(b) for b in np.argwhere(~(q == ref[0]))[:, 0]}))


# ------------------------------------------------------------------------------------- every reachable instantiation
@pytest.mark.parametrize("K,own", _reachable(), ids=["K{}-own{}".format(*p) for p in _reachable()])
@pytest.mark.parametrize("A", [2, 3, 4, 5, 6])
def test_cluster_every_instantiation_at_slice_edges(ctx, monkeypatch, A, K, own):
    """vi_det_batch_cluster<A, OWN> at K workgroups per MDP, S at the edges of its slices (first S of OWN, full slices, a ragged
    last slice, empty last parts): Q and sweeps of N sequential oracle solves.  Per S: gamma 0.9 to each MDP's own exit (terminal
    flags on every other S), then gamma 1.0 / iterations 1 / iterations 2 in turn; N = 3, 5 or 9 (never a multiple of 8)."""
    from oracle import oracle
    monkeypatch.setenv("MP_VI_BATCH_NO_REG", "1")          # (small S would take the register form)
    monkeypatch.setenv("MP_VI_BATCH_CLUSTER", str(K))
    variant = "vi_batch_cluster{}".format(K)
    for i, S in enumerate(_edges(K, own)):
        assert _takes_cluster(S, K, own) and not _takes_cluster(S, K, own - 1), (S, K, own)
        n = (3, 5, 9)[(A + own + i) % 3]
        tr, rw, tm = _tables(n, S, A, seed=1000 * A + 100 * K + 10 * own + i, terminal=i % 2 == 0)
        model = ctx.load_table_batch(tr, rw, tm)
        gamma2, iters2 = ((1.0, 200), (0.9, 1), (0.9, 2))[(A + K + own + i) % 3]
        for gamma, iters in ((0.9, 200), (gamma2, iters2)):
            ref = oracle.vi_solve_each(tr, rw, tm, gamma=gamma, iterations=iters)
            _check_device(ctx, model, gamma, iters, ref, variant)
            _check_host(ctx, model, gamma, iters, ref, variant)
            if iters == 200 and gamma < 1.0:
                assert len(set(ref[1].tolist())) > 1, ref[1]          # the MDPs of one launch stop at different sweeps
        model.close()


@pytest.mark.parametrize("K,S", [(K, _last_cluster(K) + 1) for K in (2, 4, 8)] + [(4, 10239), (8, 10239)])
@pytest.mark.parametrize("A", [2, 6])
def test_cluster_first_shape_past_the_limit(ctx, monkeypatch, A, K, S):
    """The first S past the cluster form (OWN = 4 at K = 2; the LDS at K = 4, 8), and S = 10 239 (16 S + 16 bytes fit the LDS
    but not with the kernel's static LDS on top: the call used to fail), with the form forced: another form solves it, exactly."""
    from oracle import oracle
    assert not _takes_cluster(S, K) and (_takes_cluster(S - 1, K) or S == 10239)
    monkeypatch.setenv("MP_VI_BATCH_NO_REG", "1")
    monkeypatch.setenv("MP_VI_BATCH_CLUSTER", str(K))
    tr, rw, tm = _tables(3, S, A, seed=77 + K + A)
    model = ctx.load_table_batch(tr, rw, tm)
    ref = oracle.vi_solve_each(tr, rw, tm, gamma=0.9, iterations=200)
    q, sw = ctx.vi_solve_batch(model, 0.9, 200)
    assert not ctx.last_kernel_variant().startswith("vi_batch_cluster"), ctx.last_kernel_variant()
    assert_vi_batch_form(ctx, 3, S, A, 200)
    np.testing.assert_array_equal(sw, ref[1])
    assert np.array_equal(q, ref[0])
    model.close()


# ------------------------------------------------------------------------------------ one workgroup of a cluster gives up
# per K: a shape at another OWN (S, |A|)
_GIVE_UP_SHAPE = {2: (5000, 3), 4: (6000, 4), 8: (900, 5)}


def _give_up_cases(S, A, seed):
    """(name, tables, iterations, give-up sweep as a function of the oracle's sweeps of MDP 0)."""
    base = _tables(3, S, A, seed, scales=[1.0, 1e-6, 1e-9])
    zero = (base[0], base[1].copy(), base[2])
    zero[1][0] = 0.0                                     # all-zero rewards: MDP 0 converges at its first sweep
    return [("first", base, 200, lambda sw: 0),
            ("middle", base, 200, lambda sw: int(sw[0]) // 2),
            ("converging", base, 200, lambda sw: int(sw[0]) - 1),     # MDP 0's last sweep
            ("iterations_limit", base, 30, lambda sw: 30 - 1),        # MDPs 0 and 1 stop at the limit
            ("one_iteration", base, 1, lambda sw: 0),
            ("zero_rewards", zero, 200, lambda sw: 0)]


@pytest.mark.parametrize("K,part", [(K, p) for K in (2, 4, 8) for p in range(K)])
def test_cluster_one_part_gives_up(ctx, monkeypatch, K, part):
    """Workgroup `part` of every cluster arrives at the give-up sweep and then leaves by the give-up exit while its partners carry
    on.  At an MDP's last sweep the partners see a complete word, finish and write their slices (and part 0 a real sweep count):
    only the MDP's give-up word, raised by whichever part gave up, sends it to the follow-up launch -- Q and sweeps of the oracle
    in both memory modes."""
    from oracle import oracle
    S, A = _GIVE_UP_SHAPE[K]
    monkeypatch.setenv("MP_VI_BATCH_NO_REG", "1")
    monkeypatch.setenv("MP_VI_BATCH_CLUSTER", str(K))
    variant = "vi_batch_cluster{}".format(K)
    assert _takes_cluster(S, K)
    for name, (tr, rw, tm), iters, sweep_of in _give_up_cases(S, A, seed=500 + K):
        model = ctx.load_table_batch(tr, rw, tm)
        decoy = ctx.load_table_batch(tr, rw + 1.0, tm)   # same shape, other Q: what a stale staging buffer would hold
        ref = oracle.vi_solve_each(tr, rw, tm, gamma=0.9, iterations=iters)
        sweep = sweep_of(ref[1])
        assert 0 <= sweep < iters
        hook = "{},{}".format(part, sweep)
        monkeypatch.setenv("MP_VI_BATCH_CLUSTER_GIVE_UP", hook)
        try:
            _check_device(ctx, model, 0.9, iters, ref, variant)
            monkeypatch.delenv("MP_VI_BATCH_CLUSTER_GIVE_UP")
            ctx.vi_solve_batch(decoy, 0.9, iters)
            monkeypatch.setenv("MP_VI_BATCH_CLUSTER_GIVE_UP", hook)
            _check_host(ctx, model, 0.9, iters, ref, variant)
        except AssertionError as e:
            raise AssertionError("case {} (give up at sweep {}; oracle sweeps {}): {}".format(name, sweep, ref[1].tolist(), e))
        monkeypatch.delenv("MP_VI_BATCH_CLUSTER_GIVE_UP")
        decoy.close()
        model.close()


@pytest.mark.parametrize("K", [2, 4, 8])
def test_cluster_one_part_of_one_mdp_gives_up(ctx, monkeypatch, K):
    """The give-up limited to MDP 4 of a batch of 9, at that MDP's last sweep, each part in turn: MDP 4 is solved again, and
    every other MDP keeps its own exact result."""
    from oracle import oracle
    S, A = _GIVE_UP_SHAPE[K]
    monkeypatch.setenv("MP_VI_BATCH_NO_REG", "1")
    monkeypatch.setenv("MP_VI_BATCH_CLUSTER", str(K))
    variant = "vi_batch_cluster{}".format(K)
    tr, rw, tm = _tables(9, S, A, seed=900 + K)
    model = ctx.load_table_batch(tr, rw, tm)
    decoy = ctx.load_table_batch(tr, rw * 2.0, tm)
    ref = oracle.vi_solve_each(tr, rw, tm, gamma=0.9, iterations=200)
    for part in range(K):
        hook = "{},{},4".format(part, int(ref[1][4]) - 1)
        monkeypatch.setenv("MP_VI_BATCH_CLUSTER_GIVE_UP", hook)
        _check_device(ctx, model, 0.9, 200, ref, variant)
        monkeypatch.delenv("MP_VI_BATCH_CLUSTER_GIVE_UP")
        ctx.vi_solve_batch(decoy, 0.9, 200)
        monkeypatch.setenv("MP_VI_BATCH_CLUSTER_GIVE_UP", hook)
        _check_host(ctx, model, 0.9, 200, ref, variant)
        monkeypatch.delenv("MP_VI_BATCH_CLUSTER_GIVE_UP")
    decoy.close()
    model.close()


def test_cluster_null_sweeps_out_through_the_c_abi(ctx, monkeypatch):
    """mp_vi_solve_batch with sweeps_out = NULL (allowed by the header) while clusters fail -- every cluster never meets, then one
    part gives up at an MDP's last sweep: the follow-up launch must not read the caller's missing status, and Q is the oracle's
    in both memory modes."""
    from oracle import oracle
    K, S, A, n = 4, 6000, 4, 5
    monkeypatch.setenv("MP_VI_BATCH_NO_REG", "1")
    monkeypatch.setenv("MP_VI_BATCH_CLUSTER", str(K))
    tr, rw, tm = _tables(n, S, A, seed=4242)
    model = ctx.load_table_batch(tr, rw, tm)
    ref = oracle.vi_solve_each(tr, rw, tm, gamma=0.9, iterations=200)
    for hook, value in ((None, None), ("MP_VI_BATCH_CLUSTER_NEVER_MEETS", "1"),
                        ("MP_VI_BATCH_CLUSTER_GIVE_UP", "{},{}".format(K - 1, int(ref[1][0]) - 1))):
        if hook:
            monkeypatch.setenv(hook, value)
        dq, _ = _nan_outputs(n, S, A)
        native._check(ctx._lib.mp_vi_solve_batch(ctx._h, model._h, 0.9, 200, 1e-5, 1e-8, native._ptr(dq), None,
                                                 native.MP_MEM_DEVICE))
        ctx.synchronize()
        assert ctx.last_kernel_variant() == "vi_batch_cluster{}".format(K)
        assert_vi_batch_form(ctx, n, S, A, 200)
        assert np.array_equal(dq.cpu().numpy().reshape(n, S, A), ref[0]), hook
        q = np.full((n, S, A), np.nan)
        native._check(ctx._lib.mp_vi_solve_batch(ctx._h, model._h, 0.9, 200, 1e-5, 1e-8, native._ptr(q), None,
                                                 native.MP_MEM_HOST))
        assert np.array_equal(q, ref[0]), hook
        if hook:
            monkeypatch.delenv(hook)
    model.close()


# ------------------------------------------------------------------------------ one workgroup of the persistent grid gives up
@pytest.fixture(scope="module")
def c2_problems(ctx):
    """The C2 shape (S = 10 000 -> the persistent kernel), plain and robust (M = 2), with the oracle's solutions."""
    from oracle import oracle
    from rl_agents_amd.envs import generators
    cfg = generators.highway_shaped(10, 10, 100, seed=0)
    t, r, term = cfg["transition"], cfg["reward"], cfg["terminal"]
    cfg2 = generators.rewire(cfg, 0.1, seed=4)
    out = {}
    for robust, (tt, rr, tm) in ((False, (t, r, term)),
                                 (True, (np.stack([t, cfg2["transition"]]), np.stack([r, cfg2["reward"] * 0.9]), None))):
        model = ctx.load_table(tt, rr, tm)
        q_ref, sw_ref = oracle.vi_solve("deterministic", tt, rr, tm, gamma=0.95, iterations=200, robust=robust)
        out[robust] = (model, q_ref, sw_ref)
    yield out
    for model, _, _ in out.values():
        model.close()


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("wg", ["first", "last"])
@pytest.mark.parametrize("when", ["sweep1", "verdict", "past"])
def test_persistent_one_workgroup_gives_up(ctx, monkeypatch, c2_problems, robust, wg, when):
    """Workgroup 0 or the last one of vi_det_persist treats its gather at one sweep as timed out (raises the timeout word, does not
    publish, does not arrive) while the others run on: at sweep 1 they notice; at j + kLag (j = the converging sweep) they read
    the converging verdict and leave with real values, so only the failing workgroup's states are NaN.  Host arrays: the call
    solves again on the chained launches -- the oracle's Q and sweeps.  Device arrays: the failure is reported.  Past j + kLag the
    hook never fires: one launch, exact results."""
    import torch
    model, q_ref, sw_ref = c2_problems[robust]
    j = sw_ref - 1
    sweep = {"sweep1": 1, "verdict": j + K_LAG, "past": j + K_LAG + 1}[when]
    n_wg = _cdiv(model.S, 256)                                   # (256 threads per workgroup, vi_persist_block)
    monkeypatch.setenv("MP_VI_PERSIST_GIVE_UP", "{},{}".format(0 if wg == "first" else n_wg - 1, sweep))
    q, sweeps = ctx.vi_solve(model, 0.95, 200, robust=robust)
    fired = when != "past"
    persist = "vi_det_persist_a5_m{}".format(2 if robust else 1)
    if fired:
        assert ctx.last_kernel_ms()[1] > 1, "the fallback runs the chained launches"
        assert_form(ctx, "vi_det_chain_a5_graph")
    else:
        assert ctx.last_kernel_ms()[1] == 1, "C2 is expected to run on the single persistent launch"
        assert_form(ctx, persist)
    assert sweeps == sw_ref and np.array_equal(q, q_ref)
    d_q = torch.full((model.S, model.A), float("nan"), dtype=torch.float64, device="cuda")
    d_sw = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.vi_solve_device(model, 0.95, 200, d_q, d_sw, robust=robust)
    ctx.synchronize()
    assert_form(ctx, persist)                                    # (device arrays: no fallback, the failure is reported)
    if fired:
        with pytest.raises(native.NativeError):
            native.check_device_sweeps(d_sw)
    else:
        assert native.check_device_sweeps(d_sw) == sw_ref and np.array_equal(d_q.cpu().numpy(), q_ref)
