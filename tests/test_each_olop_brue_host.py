"""OLOP and BRUE on one MDP per root (mp_olop_plan_models / mp_brue_plan_models): what the host decides without a device --
the names of the forms, and mp_each_form_info, the function the launch code itself calls for the form, the LDS bytes and the
grid (rl_agents_amd/csrc/each_host.hpp)."""
import pytest

from rl_agents_amd import native

LDS = 160 * 1024            # bytes of LDS of a compute unit (csrc/common.hpp kLdsBytes): what fits, what the knob can force
DEFAULT = LDS // 16         # the most bytes of a workgroup that take the LDS form by default: the footprint it was measured at
REC = 16                    # bytes of a packed transition record
HIGHWAY_PER_CU = dict(olop=(160 * 1024) // (32 + 9600), brue=(160 * 1024) // (80 + 9600))     # horizon 5: 17 and 16


def arrays(planner, horizon):
    """The kernel's own LDS arrays: OLOP's path[L + 1] int32, BRUE's rew[H] f64 + po[H] int2; 16-byte rounded."""
    raw = (horizon + 1) * 4 if planner == "olop" else horizon * 16
    return (raw + 15) // 16 * 16


@pytest.fixture
def no_knob(monkeypatch):
    monkeypatch.delenv("MP_EACH_MODEL", raising=False)


def test_names(no_knob):
    names = native.each_form_names()
    assert names == ["olop_each_lds", "olop_each_lds_slots", "olop_each_global", "olop_each_global_slots",
                     "brue_each_lds", "brue_each_lds_slots", "brue_each_global", "brue_each_global_slots"]
    assert not set(names) & set(native.kernel_form_names())
    for symbol in ("mp_olop_plan_models", "mp_brue_plan_models", "mp_each_form_info", "mp_each_form_names"):
        assert symbol in native.SIGNATURES
    assert len(native.SIGNATURES["mp_olop_plan_models"][1]) == len(native.SIGNATURES["mp_olop_plan"][1]) + 1
    assert len(native.SIGNATURES["mp_brue_plan_models"][1]) == len(native.SIGNATURES["mp_brue_plan"][1]) + 1


@pytest.mark.parametrize("planner", ["olop", "brue"])
def test_lds_bytes_and_grid(no_knob, planner):
    for s_each, a, h, n, cus in [(120, 5, 5, 65536, 256), (120, 5, 5, 7, 256), (6, 2, 2, 1000, 256), (1000, 3, 9, 9000, 256),
                                 (2000, 5, 4, 9000, 104), (12, 70, 70, 3, 256)]:
        info = native.each_form_info(planner, s_each, a, h, n, cus)
        need = arrays(planner, h) + s_each * a * REC
        assert info["lds_bytes"] == need and info["default_limit"] == DEFAULT and info["fit_limit"] == LDS
        # the default: a footprint that leaves 16 wavefronts to a compute unit; BRUE only while every root is resident at once
        lds_per_cu = min(32, LDS // need) if need <= LDS else 0
        assert info["lds"] == (need <= DEFAULT and (planner == "olop" or n <= cus * lds_per_cu))
        assert info["launch_lds_bytes"] == (need if info["lds"] else arrays(planner, h))
        assert info["grid"] == min(n, cus * (lds_per_cu if info["lds"] else 32))
    # the highway shape: 9.6 KB of records, 17 (OLOP) / 16 (BRUE) workgroups of the LDS form to a compute unit, 32 of the global
    info = native.each_form_info(planner, 120, 5, 5, 256 * HIGHWAY_PER_CU[planner], 256)
    assert info["lds"] and info["grid"] == 256 * HIGHWAY_PER_CU[planner]
    info = native.each_form_info(planner, 120, 5, 5, 256 * HIGHWAY_PER_CU[planner] + 1, 256)
    assert info["lds"] == (planner == "olop") and info["grid"] == 256 * HIGHWAY_PER_CU[planner] + (planner == "brue")


@pytest.mark.parametrize("planner", ["olop", "brue"])
def test_the_largest_table_that_takes_the_lds_form(monkeypatch, planner):
    """By default: the largest S_each at |A| = 3 within the measured footprint, and the next one.  Forced: the largest that
    fits a compute unit's LDS, and the next one, where the knob is ignored."""
    h = 6
    for knob, limit in ((None, DEFAULT), ("lds", LDS)):
        if knob:
            monkeypatch.setenv("MP_EACH_MODEL", knob)
        else:
            monkeypatch.delenv("MP_EACH_MODEL", raising=False)
        s_max = (limit - arrays(planner, h)) // (3 * REC)
        fits, over = native.each_form_info(planner, s_max, 3, h, 100, 256), native.each_form_info(planner, s_max + 1, 3, h, 100, 256)
        assert fits["lds"] and fits["lds_bytes"] <= limit and fits["grid"] == 100
        assert not over["lds"] and over["lds_bytes"] > limit and over["launch_lds_bytes"] == arrays(planner, h)
        assert native.each_form_info(planner, s_max + 1, 3, h, 100000, 256)["grid"] == 256 * 32
    assert native.each_form_info(planner, s_max, 3, h, 1000, 256)["grid"] == 256       # forced: one such workgroup to a compute unit


@pytest.mark.parametrize("planner", ["olop", "brue"])
def test_knob(monkeypatch, planner):
    monkeypatch.setenv("MP_EACH_MODEL", "global")
    info = native.each_form_info(planner, 120, 5, 5, 65536, 256)
    assert not info["lds"] and info["grid"] == 256 * 32 and info["launch_lds_bytes"] == arrays(planner, 5)
    assert info["lds_bytes"] == arrays(planner, 5) + 120 * 5 * REC
    monkeypatch.setenv("MP_EACH_MODEL", "lds")
    info = native.each_form_info(planner, 120, 5, 5, 65536, 256)          # (BRUE's default at this batch size is the global form)
    assert info["lds"] and info["grid"] == 256 * HIGHWAY_PER_CU[planner]
    big = native.each_form_info(planner, 1000, 3, 5, 65536, 256)           # 48 000 bytes: beyond the default, forced
    assert big["lds"] and big["grid"] == 256 * 3
    too_big = native.each_form_info(planner, 4000, 3, 5, 65536, 256)          # 192 000 bytes of records: the knob is ignored
    assert not too_big["lds"] and too_big["grid"] == 256 * 32


def test_bad_arguments():
    with pytest.raises(Exception):
        native.each_form_info("olop", 0, 3, 5, 10)
    with pytest.raises(KeyError):
        native.each_form_info("opd", 10, 3, 5, 10)
