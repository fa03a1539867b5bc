"""CPU tests of the batched value iteration's choice of kernel form (mp_vi_batch_geometry: vi_batch_geometry, the function
mp_vi_solve_batch launches from, run on the host alone).

  * cases derived by hand from the dispatcher this function replaced, form by form;
  * a sweep over device sizes, batch sizes, state counts at every edge, |A| and knob settings against ``_ladder`` below: the
    ladder of that dispatcher restated as a table of rungs (written from its source, not from vi_batch_geometry), with the one
    deliberate difference that a forced MP_VI_BATCH_CLUSTER other than 2, 4 or 8 means one workgroup per MDP;
  * the (K, OWN) pairs of the cluster form tests/test_gpu_vi_cluster.py parametrizes over;
  * the errors."""
import ctypes as C

import numpy as np
import pytest

from rl_agents_amd import native

KNOBS = ("MP_VI_BATCH_NO_REG", "MP_VI_BATCH_NO_WGR", "MP_VI_BATCH_NO_VLDS", "MP_VI_BATCH_CLUSTER",
         "MP_VI_BATCH_CLUSTER_NEVER_MEETS", "MP_VI_BATCH_CLUSTER_GIVE_UP")
REG = ((1, 64), (2, 64), (2, 128), (2, 256), (4, 256), (4, 512), (4, 1024))
NAMES = ["vi_batch_reg<{},{}>".format(*f) for f in REG] + ["vi_batch_cluster2", "vi_batch_cluster4", "vi_batch_cluster8",
                                                           "vi_batch_wg_stream", "vi_batch_wg_lds", "vi_batch_wg_global"]


def _set_knobs(monkeypatch, knobs):
    """knobs: {"NO_REG": 1, "CLUSTER": 4, ...} -> the MP_VI_BATCH_* variables, every other one unset."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("MP_VI_BATCH_" + k, str(v))


# ------------------------------------------------------------------------------------------------------------- pinned cases
# (N, Sb, A, iterations, knobs) -> name and the fields worth pinning; 256 compute units
PINNED = [
    ((4096, 120, 5, 200, {}), "vi_batch_reg<2,64>", {}),
    ((3, 64, 3, 200, {}), "vi_batch_reg<1,64>", {}),
    ((3, 65, 2, 200, {}), "vi_batch_reg<2,64>", {}),
    ((3, 2049, 4, 200, {}), "vi_batch_reg<4,1024>", {}),
    ((3, 2049, 5, 200, {}), "vi_batch_cluster8", dict(own=1)),
    ((3, 2049, 8, 200, {}), "vi_batch_wg_stream", {}),
    ((200, 2049, 5, 200, {}), "vi_batch_wg_stream", {}),
    ((3, 4097, 4, 200, {}), "vi_batch_cluster8", {}),
    ((64, 10000, 5, 200, {}), "vi_batch_cluster4", dict(own=3, grid=256, lds=160016)),
    ((32, 10000, 5, 200, {}), "vi_batch_cluster8", dict(own=2, grid=256)),
    ((33, 10000, 5, 200, {}), "vi_batch_cluster4", dict(grid=160)),
    ((65, 10000, 5, 200, {}), "vi_batch_wg_stream", {}),                      # (K = 2 would need own 5)
    ((256, 10000, 5, 200, {}), "vi_batch_wg_stream", dict(lds=160000)),
    ((3, 10000, 7, 200, {}), "vi_batch_wg_lds", {}),
    ((3, 10207, 5, 200, {}), "vi_batch_cluster8", {}),
    ((3, 10208, 5, 200, {}), "vi_batch_wg_stream", {}),
    ((3, 10209, 5, 200, {}), "vi_batch_wg_global", {}),
    ((3, 10000, 5, 0, {}), "vi_batch_wg_stream", {}),
    ((3, 6144, 5, 200, dict(NO_REG=1, CLUSTER=2)), "vi_batch_cluster2", dict(own=3)),
    ((3, 6145, 5, 200, dict(NO_REG=1, CLUSTER=2)), "vi_batch_wg_stream", {}),
    ((3, 10000, 5, 200, dict(CLUSTER=3)), "vi_batch_wg_stream", {}),
    # test_vi_batch_workgroup_forms' small shape, with the knobs it sets: without MP_VI_BATCH_CLUSTER=0 the cluster rung comes
    # first for 21 MDPs on 256 compute units (21 * 8 <= 256), as it always has -- no other knob switches that rung off
    ((21, 30, 4, 200, dict(NO_REG=1, NO_WGR=1, CLUSTER=0)), "vi_batch_wg_lds", {}),
    ((21, 30, 4, 200, dict(NO_REG=1, NO_VLDS=1, CLUSTER=0)), "vi_batch_wg_global", {}),
    ((21, 30, 4, 200, dict(NO_REG=1, NO_WGR=1)), "vi_batch_cluster8", dict(own=1)),
    ((21, 30, 4, 200, dict(NO_REG=1, NO_VLDS=1)), "vi_batch_cluster8", dict(own=1)),
    ((300, 30, 4, 200, dict(NO_REG=1, NO_WGR=1)), "vi_batch_wg_lds", {}),
    ((300, 30, 4, 200, dict(NO_REG=1, NO_VLDS=1)), "vi_batch_wg_global", {}),
]


@pytest.mark.parametrize("case,name,fields", PINNED, ids=["{}x{}xA{}-it{}-{}".format(*c[:4], "-".join(sorted(c[4])) or "default")
                                                          for c, _, _ in PINNED])
def test_pinned_cases(monkeypatch, case, name, fields):
    N, Sb, A, iters, knobs = case
    _set_knobs(monkeypatch, knobs)
    g = native.vi_batch_geometry(N, Sb, A, iters, cus=256)
    assert g["name"] == name, g
    assert {k: g[k] for k in fields} == fields, g


# ---------------------------------------------------------------------------------------------------------------- the sweep
LDS_BYTES = 160 * 1024
LDS_MARGIN = 512
UNROLLED = (2, 3, 4, 5, 6, 8)
VLDS_OWN = 10


def _cdiv(a, b):
    return -(-a // b)


def _ladder(cus, N, Sb, A, iters, knobs):
    """The rungs in order, each (holds, fields): the first that holds is taken."""
    at = A if A in UNROLLED else 0
    v2 = 16 * Sb                                           # V_k and V_{k+1} in LDS
    if "CLUSTER" in knobs:
        K = knobs["CLUSTER"] if knobs["CLUSTER"] in (2, 4, 8) else 1
    else:
        K = 1
        while K < 8 and N * 2 * K <= cus:
            K *= 2
    c_own = _cdiv(_cdiv(Sb, K), 1024)
    vlds = Sb <= VLDS_OWN * 1024 and v2 <= LDS_BYTES - LDS_MARGIN and "NO_VLDS" not in knobs
    rungs = [(at > 0 and "NO_REG" not in knobs and Sb <= own * block and ((own, block) != (4, 1024) or at <= 4),
              dict(form="reg", name="vi_batch_reg<{},{}>".format(own, block), own=own, block=block, k=1, grid=N, lds=v2))
             for own, block in REG]
    rungs.append((2 <= at <= 6 and iters > 0 and K > 1 and c_own <= 3 and v2 + 16 <= LDS_BYTES - LDS_MARGIN,
                  dict(form="cluster", name="vi_batch_cluster{}".format(K), own=c_own, block=1024, k=K, grid=_cdiv(N, 8) * 8 * K,
                       lds=v2 + 16)))
    rungs.append((at > 0 and vlds and "NO_WGR" not in knobs,
                  dict(form="wg_stream", name="vi_batch_wg_stream", own=0, block=1024, k=1, grid=N, lds=v2)))
    rungs.append((vlds, dict(form="wg_lds", name="vi_batch_wg_lds", own=0, block=1024, k=1, grid=N, lds=v2)))
    rungs.append((True, dict(form="wg_global", name="vi_batch_wg_global", own=0, block=1024, k=1, grid=N, lds=0)))
    for holds, fields in rungs:
        if holds:
            return dict(fields, at=at)


def _state_counts():
    """Both sides of every edge of the ladder: the register forms' ranges, the cluster's slices (K * 1024 * OWN), the LDS bound
    with and without the cluster's 16 bytes, the VLDS forms' 10 * 1024."""
    edges = {1, 30} | {own * block for own, block in REG} | {K * 1024 * own for K in (2, 4, 8) for own in (1, 2, 3)}
    edges |= {(LDS_BYTES - LDS_MARGIN) // 16, (LDS_BYTES - LDS_MARGIN - 16) // 16, VLDS_OWN * 1024}
    return sorted(edges | {e + 1 for e in edges})


KNOB_SETS = [{}, dict(NO_REG=1), dict(NO_WGR=1), dict(NO_VLDS=1)] + \
            [dict(base, CLUSTER=k) for k in (0, 1, 2, 3, 4, 8, 16) for base in ({}, dict(NO_REG=1))]


def test_sweep_against_the_ladder(monkeypatch):
    """Every field of the query over the grid of the module docstring.  iterations matters to the cluster rung alone (> 0), so
    0 and 1 run where that rung can hold: |A| = 5 and |A| = 7."""
    names, pairs, n, bad = set(), set(), 0, []
    for knobs in KNOB_SETS:
        _set_knobs(monkeypatch, knobs)
        for cus in (8, 64, 256, 304):
            for N in (1, 4, 5, 16, 17, 32, 33, 64, 65, 128, 129, 4096):
                for Sb in _state_counts():
                    for A in range(1, 10):
                        for iters in ((0, 1, 200) if A in (5, 7) else (200,)):
                            got = native.vi_batch_geometry(N, Sb, A, iters, cus=cus)
                            want = _ladder(cus, N, Sb, A, iters, knobs)
                            n += 1
                            if got != want:
                                bad.append(((cus, N, Sb, A, iters, knobs), want, got))
                            names.add(got["name"])
                            if got["form"] == "cluster":
                                pairs.add((got["k"], got["own"]))
    assert not bad, "{} of {} queries differ, e.g. {}".format(len(bad), n, bad[:3])
    assert sorted(names) == sorted(NAMES)
    assert set(NAMES) <= set(native.kernel_form_names())
    assert sorted(pairs) == [(2, 1), (2, 2), (2, 3), (4, 1), (4, 2), (4, 3), (8, 1), (8, 2)]


def test_cluster_cases_of_the_gpu_tests(monkeypatch):
    """tests/test_gpu_vi_cluster.py takes its (K, OWN) pairs and state counts from the query: they are the ones it ran on when
    it carried its own copy of the dispatcher's formulas."""
    from tests import test_gpu_vi_cluster as t
    _set_knobs(monkeypatch, dict(CLUSTER=16, NO_VLDS=1))            # (it sets its own knobs, whatever the process has)
    assert {p: t._edges(*p) for p in t._reachable()} == {
        (2, 1): [1, 2047, 2048], (2, 2): [2049, 4095, 4096], (2, 3): [4097, 6143, 6144],
        (4, 1): [1, 5, 4093, 4096], (4, 2): [4097, 8189, 8192], (4, 3): [8193, 10205],
        (8, 1): [1, 9, 8185, 8192], (8, 2): [8193, 10201]}
    assert [t._last_cluster(K) + 1 for K in (2, 4, 8)] == [6145, 10208, 10208]
    assert native.vi_batch_geometry(3, 10000, 5, 200)["name"] == "vi_batch_wg_global"      # (the knobs are back)


def test_knobs_are_read_at_each_call(monkeypatch):
    _set_knobs(monkeypatch, {})
    assert native.vi_batch_geometry(3, 10000, 5, 200)["name"] == "vi_batch_cluster8"
    _set_knobs(monkeypatch, dict(CLUSTER=0))
    assert native.vi_batch_geometry(3, 10000, 5, 200)["name"] == "vi_batch_wg_stream"
    _set_knobs(monkeypatch, {})
    assert native.vi_batch_geometry(3, 10000, 5, 200)["name"] == "vi_batch_cluster8"


def test_errors(monkeypatch):
    """A NULL argument and a size below 1 are refused; iterations may be 0, not negative."""
    _set_knobs(monkeypatch, {})
    lib = native.load()
    out, name = np.zeros(7, np.int64), C.c_char_p()
    assert lib.mp_vi_batch_geometry(3, 100, 5, 200, 256, None, C.byref(name)) == native.ERR_ARG
    assert lib.mp_vi_batch_geometry(3, 100, 5, 200, 256, native._ptr(out), None) == native.ERR_ARG
    for bad in ((0, 100, 5, 200, 256), (3, 0, 5, 200, 256), (3, 100, 0, 200, 256), (3, 100, 5, -1, 256), (3, 100, 5, 200, 0)):
        with pytest.raises(native.NativeError) as e:
            native.vi_batch_geometry(*bad[:4], cus=bad[4])
        assert e.value.code == native.ERR_ARG
    assert native.vi_batch_geometry(3, 100, 5, 0)["name"] == "vi_batch_reg<2,64>"
