"""Sparse Sampling on one MDP per root (mp_ss_plan_models): what the host decides without a device -- the names of the forms
and mp_each_form_info, the function the launch code itself calls for the form, the LDS bytes and the grid
(rl_agents_amd/csrc/each_host.hpp) -- and the fixture of the unmodified reference (tests/golden/per_episode_sparse_sampling.npz)
against the restatement the GPU tests compare the device with (tests/sparse_sampling_restatement.py)."""
import os

import numpy as np
import pytest

from rl_agents_amd import native
from tests import sparse_sampling_restatement as sr
from tests.helpers import generator_from

LDS = 160 * 1024            # bytes of LDS of a compute unit (csrc/common.hpp kLdsBytes): what fits, what the knob can force
DEFAULT = LDS // 16         # the most bytes of a workgroup that take the LDS form by default: the footprint it was measured at
REC = 16                    # bytes of a packed transition record
FRAME = 64                  # bytes of a frame on a table: 56 + one (state, count) list entry
HERE = os.path.dirname(os.path.abspath(__file__))


def frames(horizon):
    return 16 * -(-horizon * FRAME // 16)


@pytest.fixture
def no_knob(monkeypatch):
    monkeypatch.delenv("MP_EACH_MODEL", raising=False)


def test_names(no_knob):
    names = native.ss_each_form_names()
    assert names == ["ss_each_lds", "ss_each_global"]
    for other in (native.kernel_form_names(), native.each_form_names(), native.ss_form_names()):
        assert not set(names) & set(other)
    for symbol in ("mp_ss_plan_models", "mp_ss_each_form_names"):
        assert symbol in native.SIGNATURES
    assert len(native.SIGNATURES["mp_ss_plan_models"][1]) == len(native.SIGNATURES["mp_ss_plan"][1]) + 1
    assert native.EACH_PLANNERS["ss"] == 2


def test_lds_bytes_and_grid(no_knob):
    for s_each, a, h, n, cus in [(120, 5, 3, 65536, 256), (120, 5, 3, 7, 256), (6, 2, 2, 1000, 256), (1000, 3, 9, 9000, 256),
                                 (2000, 5, 4, 9000, 104), (12, 70, 16, 3, 256)]:
        info = native.each_form_info("ss", s_each, a, h, n, cus)
        need = frames(h) + s_each * a * REC
        assert info["lds_bytes"] == need and info["default_limit"] == DEFAULT and info["fit_limit"] == LDS
        # the default (profiles/ss_each_ab.json): a footprint that leaves 16 wavefronts to a compute unit, and only while every
        # root's workgroup is resident at once
        lds_per_cu = min(32, LDS // need) if need <= LDS else 0
        assert info["lds"] == (need <= DEFAULT and n <= cus * lds_per_cu)
        assert info["launch_lds_bytes"] == (need if info["lds"] else frames(h))
        assert info["grid"] == min(n, cus * (lds_per_cu if info["lds"] else 32))
    # the highway shape at horizon 3: 192 bytes of frames + 9.6 KB of records, 16 workgroups of the LDS form to a compute unit
    per_cu = LDS // (192 + 9600)
    assert per_cu == 16
    info = native.each_form_info("ss", 120, 5, 3, 256 * per_cu, 256)
    assert info["lds"] and info["grid"] == 256 * per_cu and info["launch_lds_bytes"] == 9792
    info = native.each_form_info("ss", 120, 5, 3, 256 * per_cu + 1, 256)
    assert not info["lds"] and info["grid"] == 256 * per_cu + 1 and info["launch_lds_bytes"] == 192


def test_the_largest_table_that_takes_the_lds_form(monkeypatch):
    """By default: the largest S_each at |A| = 3 within the measured footprint, and the next one.  Forced: the largest that
    fits a compute unit's LDS, and the next one, where the knob is ignored."""
    h = 6
    for knob, limit in ((None, DEFAULT), ("lds", LDS)):
        if knob:
            monkeypatch.setenv("MP_EACH_MODEL", knob)
        else:
            monkeypatch.delenv("MP_EACH_MODEL", raising=False)
        s_max = (limit - frames(h)) // (3 * REC)
        fits, over = native.each_form_info("ss", s_max, 3, h, 100, 256), native.each_form_info("ss", s_max + 1, 3, h, 100, 256)
        assert fits["lds"] and fits["lds_bytes"] <= limit and fits["grid"] == 100
        assert not over["lds"] and over["lds_bytes"] > limit and over["launch_lds_bytes"] == frames(h)
        assert native.each_form_info("ss", s_max + 1, 3, h, 100000, 256)["grid"] == 256 * 32
    assert native.each_form_info("ss", s_max, 3, h, 1000, 256)["grid"] == 256       # forced: one such workgroup to a compute unit


def test_knob(monkeypatch):
    monkeypatch.setenv("MP_EACH_MODEL", "global")
    info = native.each_form_info("ss", 120, 5, 3, 256, 256)             # (the default at this batch size is the LDS form)
    assert not info["lds"] and info["grid"] == 256 and info["launch_lds_bytes"] == 192
    assert info["lds_bytes"] == 192 + 120 * 5 * REC
    monkeypatch.setenv("MP_EACH_MODEL", "lds")
    info = native.each_form_info("ss", 120, 5, 3, 65536, 256)           # (the default at this batch size is the global form)
    assert info["lds"] and info["grid"] == 256 * 16
    big = native.each_form_info("ss", 1000, 3, 3, 65536, 256)            # 48 192 bytes: beyond the default, forced
    assert big["lds"] and big["grid"] == 256 * 3
    too_big = native.each_form_info("ss", 4000, 3, 3, 65536, 256)        # 192 000 bytes of records: the knob is ignored
    assert not too_big["lds"] and too_big["grid"] == 256 * 32


def test_bad_arguments():
    with pytest.raises(native.NativeError):
        native.each_form_info("ss", 0, 3, 3, 10)
    with pytest.raises(native.NativeError):
        native.each_form_info("ss", 10, 3, 3, 0)
    with pytest.raises(KeyError):
        native.each_form_info("sparse_sampling", 10, 3, 3, 10)
    out = np.zeros(6, np.int64)
    assert native.load().mp_each_form_info(3, 10, 3, 3, 10, 256, out.ctypes.data) == native.MP_ERR_ARG


def test_the_fixture_equals_the_restatement_step_by_step():
    """Every plan, every generator record and every root value (by bits) of the unmodified reference's per-episode agents: this
    pins the fixture and the restatement to each other without a GPU."""
    z = np.load(os.path.join(HERE, "golden", "per_episode_sparse_sampling.npz"))
    horizon, n_samples, gamma = int(z["ss/horizon"]), int(z["ss/C"]), float(z["ss/gamma"])
    assert (horizon, n_samples, gamma) == (3, 2, 0.8)
    n = len(z["s0"])
    lengths, ties = [], 0
    for e in range(n):
        steps = int(z["ss/e{}/n_steps".format(e)])
        lengths.append(steps)
        assert int(z["ss/e{}/states".format(e)][0]) == int(z["s0"][e])
        record = z["ss/e{}/rng_before".format(e)]
        for t in range(steps):
            p = "ss/e{}/t{}".format(e, t)
            np.testing.assert_array_equal(record, z[p + "/rng_before"], err_msg=p)      # the stream runs on from plan to plan
            gen = generator_from(record)
            res = sr.ss_plan("deterministic", z["transition"][e, t], z["reward"][e, t], int(z["ss/e{}/states".format(e)][t]), horizon,
                             n_samples, gamma, gen)
            assert res["plan"].tolist() == z[p + "/plan"].tolist(), p
            record = native.rng_state_from_generator(gen)
            np.testing.assert_array_equal(record, z[p + "/rng_after"], err_msg=p)
            assert np.float64(res["root_value"]).view(np.uint64) == np.float64(z[p + "/root_value"]).view(np.uint64), p
            values = res["root_values"]
            assert int((values == values.max()).sum()) == int(z[p + "/root_ties"]), p
            ties = max(ties, int(z[p + "/root_ties"]))
            assert int(z[p + "/env_steps_total"]) == 0                                 # planner.observations stays empty
    assert ties >= 2 and min(lengths) < max(lengths) == 3     # the tie draw and an episode that ends early are in the fixture
