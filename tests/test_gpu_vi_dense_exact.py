"""Dense value iteration in numpy's own summation order (mp_vi_dense_mode(MP_VI_DENSE_EXACT), vi_dense_exact_q):
BIT-EXACT against the reference's goldens and the pinned oracle -- Q, V and sweep counts -- where the matrix-core form
is compared at 1e-12 with a sweep count within one (tests/test_gpu_golden.py, tests/test_gpu_batch.py).

value_iteration.py:54-55 computes (T * v.reshape(1, 1, S)).sum(axis=-1): every product rounded, then numpy's pairwise
add.reduce (eight strided accumulators per block of at most 128 elements, halving recursion above).  The row lengths
below walk every shape of that recursion: fewer than 8 elements, one block with and without a remainder, two unequal
halves, several levels, a remainder in the last block only.
"""
import numpy as np
import pytest

from tests.helpers import assert_form, mdp_from_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    c.vi_dense_mode("exact")
    yield c
    c.close()


def test_goldens_dense_bit_exact(ctx, golden):
    """Every stochastic-mode case of the reference's own outputs, VI and robust VI."""
    z = golden["vi"]
    seen = 0
    for name in [str(n) for n in z["vi/names"]]:
        p = "vi/" + name
        cfg = mdp_from_golden(z, p + "/mdp")
        if cfg["mode"] != "stochastic":
            continue
        model = ctx.load_dense(cfg["transition"], cfg["reward"], cfg["terminal"])
        gamma, iters = float(z[p + "/gamma"]), int(z[p + "/iterations"])
        q, sweeps = ctx.vi_solve(model, gamma, iters)
        v = ctx.vi_solve_v(model, gamma, iters)
        assert sweeps == int(z[p + "/sweeps"]), name
        assert np.array_equal(q, z[p + "/Q"]), name
        assert np.array_equal(v, z[p + "/V"]), name
        model.close()
        seen += 1
    for name in [str(n) for n in z["rvi/names"]]:
        p = "rvi/" + name
        if str(z[p + "/mode"]) == "deterministic":
            continue
        model = ctx.load_dense(z[p + "/transitions"], z[p + "/rewards"])
        q, sweeps = ctx.vi_solve(model, float(z[p + "/gamma"]), int(z[p + "/iterations"]), robust=True)
        assert sweeps == int(z[p + "/sweeps"]), name
        assert np.array_equal(q, z[p + "/Q"]), name
        model.close()
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("s,a", [(1, 2), (5, 3), (7, 2), (8, 2), (17, 2), (64, 3), (100, 4), (128, 2), (129, 2), (131, 3),
                                 (257, 3), (333, 5), (1029, 2), (2500, 3), (4099, 2)])
def test_vs_oracle_all_recursion_shapes(ctx, s, a):
    from oracle import oracle
    from rl_agents_amd.envs import generators
    cfg = generators.random_stochastic(s, a, seed=s, terminal_rate=0.1)
    model = ctx.load_dense(cfg["transition"], cfg["reward"], cfg["terminal"])
    q, sweeps = ctx.vi_solve(model, 0.9, 40)
    q_ref, sweeps_ref = oracle.vi_solve("stochastic", cfg["transition"], cfg["reward"], cfg["terminal"], gamma=0.9,
                                        iterations=40)
    assert sweeps == sweeps_ref
    assert np.array_equal(q, q_ref)
    v = ctx.vi_solve_v(model, 0.9, 40)
    v_ref = oracle.vi_solve("stochastic", cfg["transition"], cfg["reward"], cfg["terminal"], gamma=0.9, iterations=40,
                            state_value=True)
    assert np.array_equal(v, v_ref)
    model.close()


def test_numpy_itself(ctx):
    """One backup against numpy's own expression (not the oracle): negative values, exact zeros, a terminal mask."""
    g = np.random.Generator(np.random.PCG64(3))
    for s in (6, 96, 777, 3000):
        t = g.random((s, 3, s))
        t[g.random((s, 3, s)) < 0.3] = 0.0
        t /= np.maximum(t.sum(-1, keepdims=True), 1e-300)
        r = g.standard_normal((s, 3))
        term = g.random(s) < 0.2
        v = g.standard_normal(s)
        model = ctx.load_dense(t, r, term)
        q = ctx.vi_backup(model, 0.95, v)
        next_v = (t * v.reshape((1, 1, v.size))).sum(axis=-1)      # value_iteration.py:54-55
        next_v[term] = 0                                            # :62
        assert np.array_equal(q, r + 0.95 * next_v), s              # :63
        model.close()


def test_robust_and_row_blocks(ctx):
    from oracle import oracle
    from rl_agents_amd.distributed import vi_solve_row_sharded
    from rl_agents_amd.envs import generators
    c1 = generators.random_stochastic(301, 3, seed=5)
    c2 = generators.random_stochastic(301, 3, seed=6)
    tt, rr = np.stack([c1["transition"], c2["transition"]]), np.stack([c1["reward"], c2["reward"]])
    both = ctx.load_dense(tt, rr)
    q, sweeps = ctx.vi_solve(both, 0.9, 60, robust=True)
    q_ref, sweeps_ref = oracle.vi_solve("stochastic", tt, rr, None, gamma=0.9, iterations=60, robust=True)
    assert sweeps == sweeps_ref and np.array_equal(q, q_ref)
    # a block of source rows reassembles the full backup, and the row-sharded driver is the same solve
    v = np.random.Generator(np.random.PCG64(1)).random(301)
    q_full = ctx.vi_backup(both, 0.9, v, robust=True)
    parts = []
    for lo, hi in ((0, 100), (100, 101), (101, 301)):
        blk = ctx.load_dense_rows(tt[:, lo:hi], rr[:, lo:hi], None)
        parts.append(ctx.vi_backup(blk, 0.9, v, robust=True))
    assert np.array_equal(np.concatenate(parts), q_full)
    assert np.array_equal(q_full, oracle.dense_backup_rows(tt, rr, None, v, 0.9, robust=True))
    q2, sweeps2 = vi_solve_row_sharded(ctx, tt, rr, None, gamma=0.9, iterations=60, robust=True)
    assert sweeps2 == sweeps_ref and np.array_equal(q2, q_ref)
    both.close()


def test_v_through_l2_and_mode_switch(ctx, monkeypatch):
    """Rows too long for V to sit in LDS beside the tables read it through L2 (forced here on a short row), and the
    matrix-core form comes back with mp_vi_dense_mode(MP_VI_DENSE_MFMA)."""
    from oracle import oracle
    from rl_agents_amd.envs import generators
    cfg = generators.random_stochastic(700, 2, seed=11, terminal_rate=0.1)
    model = ctx.load_dense(cfg["transition"], cfg["reward"], cfg["terminal"])
    q_ref, sweeps_ref = oracle.vi_solve("stochastic", cfg["transition"], cfg["reward"], cfg["terminal"], gamma=0.9,
                                        iterations=30)
    from rl_agents_amd import native
    nbt = native.vi_geometry("stochastic", Sc=700)["nbt"]
    monkeypatch.setenv("MP_VI_EXACT_NO_VLDS", "1")
    q, sweeps = ctx.vi_solve(model, 0.9, 30)
    assert_form(ctx, "vi_dense_exact_n{}_global".format(nbt))
    assert sweeps == sweeps_ref and np.array_equal(q, q_ref)
    monkeypatch.delenv("MP_VI_EXACT_NO_VLDS")
    monkeypatch.setenv("MP_VI_EXACT_V", "pieces")
    q, sweeps = ctx.vi_solve(model, 0.9, 30)
    assert_form(ctx, "vi_dense_exact_n{}_pieces".format(nbt))
    assert sweeps == sweeps_ref and np.array_equal(q, q_ref)
    monkeypatch.delenv("MP_VI_EXACT_V")
    monkeypatch.setenv("MP_VI_EXACT_WAVES", "4")
    assert native.vi_geometry("stochastic", Sc=700)["waves"] == 4
    q, sweeps = ctx.vi_solve(model, 0.9, 30)
    assert_form(ctx, "vi_dense_exact_n{}_lds".format(nbt))
    assert sweeps == sweeps_ref and np.array_equal(q, q_ref)
    monkeypatch.delenv("MP_VI_EXACT_WAVES")
    assert native.vi_geometry("stochastic", Sc=700)["waves"] == 8
    ctx.vi_dense_mode("mfma")
    try:
        q_m, sweeps_m = ctx.vi_solve(model, 0.9, 30)
        assert_form(ctx, "vi_dense_mfma")
        np.testing.assert_allclose(q_m, q_ref, rtol=1e-12, atol=1e-12)
        assert abs(sweeps_m - sweeps_ref) <= 1
    finally:
        ctx.vi_dense_mode("exact")
    q, sweeps = ctx.vi_solve(model, 0.9, 30)
    assert_form(ctx, "vi_dense_exact_n{}_lds".format(nbt))
    assert sweeps == sweeps_ref and np.array_equal(q, q_ref)
    model.close()


@pytest.mark.parametrize("s_cols,v_mode", [(8193, None), (10000, "pieces"), (10000, "global"), (16385, None), (50000, None)])
def test_rows_longer_than_numpys_reduction_buffer(ctx, monkeypatch, s_cols, v_mode):
    """Rows of more than 8192 next states: numpy's add.reduce is the running sum of the pairwise sums of 8192-element
    pieces (tests/test_oracle_vi_long_rows.py pins the oracle on numpy for it).  A block of source rows of such a model
    (the unit of the row-sharded solve), two models, against numpy's own expression and the oracle; 50 000 columns take
    the kernel form that stages V piece by piece (it no longer fits LDS beside the tables: native.vi_geometry), forced on
    10 000 as well, where reading V through L2 is forced too; the form of each is asserted."""
    from oracle import oracle
    g = np.random.Generator(np.random.PCG64(s_cols))
    rows, a = 37, 2
    t = g.random((2, rows, a, s_cols))
    t /= t.sum(-1, keepdims=True)
    r = g.random((2, rows, a))
    v = g.standard_normal(s_cols) * 3
    if v_mode:
        monkeypatch.setenv("MP_VI_EXACT_V", v_mode)
    from rl_agents_amd import native
    geo = native.vi_geometry("stochastic", Sc=s_cols)       # (read with the knob set: the placement the launch takes)
    assert geo["v"] == (v_mode or geo["v_default"]) and geo["v_default"] == ("pieces" if s_cols == 50000 else "lds")
    form = "vi_dense_exact_n{}_{}".format(geo["nbt"], geo["v"])
    blk = ctx.load_dense_rows(t, r, None)
    q = ctx.vi_backup(blk, 0.95, v, robust=True)
    assert_form(ctx, form)
    ref = np.min(r + 0.95 * (t * v.reshape((1, 1, 1, v.size))).sum(axis=-1), axis=0)   # robust_value_iteration.py:46-58
    assert np.array_equal(q, ref)
    assert np.array_equal(q, oracle.dense_backup_rows(t, r, None, v, 0.95, robust=True))
    blk.close()
    term = g.random(rows) < 0.3
    one = ctx.load_dense_rows(t[0], r[0], term)
    q1 = ctx.vi_backup(one, 0.95, v)
    assert_form(ctx, form)
    next_v = (t[0] * v.reshape((1, 1, v.size))).sum(axis=-1)
    next_v[term] = 0
    assert np.array_equal(q1, r[0] + 0.95 * next_v)
    one.close()
