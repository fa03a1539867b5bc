"""The tree exports of the wave-per-root planners (mp_olop_tree_export, mp_brue_tree_export, mp_ss_tree_export) on the part of
their contract that their heads share (csrc/wave_host.hpp) and the one place where they differ on purpose: an export refused
for its capacity leaves *n_nodes alone after OLOP and BRUE, and holds the node count after Sparse Sampling (include/mi355plan.h:
that call is how a caller sizes its arrays)."""
import ctypes as C

import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.envs import generators

pytestmark = pytest.mark.gpu

N_ROOTS = 4
EXPORTS = {"olop": ("mp_olop_tree_export", 9), "brue": ("mp_brue_tree_export", 6), "ss": ("mp_ss_tree_export", 6)}


def raw_export(ctx, planner, root, cap, preset):
    """(return code, error text, *n_nodes) of the planner's export with every array NULL and *n_nodes preset."""
    name, n_arrays = EXPORTS[planner]
    n = C.c_int32(preset)
    rc = getattr(ctx._lib, name)(ctx._h, root, cap, C.byref(n), *([None] * n_arrays))
    return rc, ctx._lib.mp_last_error().decode("utf-8", "replace"), n.value


def test_export_heads_and_the_count_of_a_refused_capacity():
    ctx = native.Context(0)
    try:
        tab = generators.random_deterministic(20, 3, seed=7)
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        s0 = np.arange(N_ROOTS, dtype=np.int32)
        plans = {
            "olop": lambda: ctx.olop_plan(model, s0, 5, 3, 0.8, True, -1, np.full(5, 4 * np.log(5)),
                                          np.array([(1 - 0.8 ** (4 - d)) / (1 - 0.8) for d in range(4)]),
                                          native.seed_sequence_states((), 1, N_ROOTS)),
            "brue": lambda: ctx.brue_plan(model, s0, 30, 3, 0.8, np.array([0.8 ** d for d in range(4)]),
                                          native.seed_sequence_states((), 1, N_ROOTS)),
            "ss": lambda: ctx.ss_plan(model, s0, 2, 2, 0.8, native.seed_sequence_states((), 1, N_ROOTS)),
        }
        full = {"olop": lambda r: ctx.olop_tree(r, 1 + 5 * 3 * 3), "brue": lambda r: ctx.brue_tree(r, 1 + 2 * (30 + 3)),
                "ss": lambda r: ctx.ss_tree(r)}
        for planner in ("olop", "brue", "ss"):
            out = plans[planner]()
            assert (out["status"] == 0).all()
            # a capacity of one node: refused, and what *n_nodes holds afterwards
            for root in range(N_ROOTS):
                rc, text, n = raw_export(ctx, planner, root, 1, -7)
                assert rc == native.MP_ERR_ARG and "capacity 1 <" in text, (planner, root, rc, text)
                if planner == "ss":
                    assert n == len(ctx.ss_tree(root)["parent"]) > 1, (root, n)
                else:
                    assert n == -7, (planner, root, n)
            # roots outside the batch
            for root in (-1, N_ROOTS):
                rc, text, n = raw_export(ctx, planner, root, 1 << 20, -7)
                assert rc == native.MP_ERR_ARG and "root" in text and "out of range" in text and n == -7, (planner, root, rc, text)
            # the other planners' exports find no tree of theirs on this ctx
            for other in EXPORTS:
                if other != planner:
                    rc, text, n = raw_export(ctx, other, 0, 1 << 20, -7)
                    assert rc == native.MP_ERR_ARG and n == -7, (planner, other, rc, text)
                    with pytest.raises(native.NativeError) as e:
                        full[other](0)
                    assert e.value.code == native.MP_ERR_ARG
            # and the last root's tree at full capacity
            tree = full[planner](N_ROOTS - 1)
            assert len(tree["parent"]) > 1 and tree["parent"][0] == -1
        model.close()
    finally:
        ctx.close()
