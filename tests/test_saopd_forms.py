"""CPU tests of the state-aware planner's choice of kernel form (mp_saopd_choose_form: sa_choose, the function mp_saopd_plan
calls, run on the host alone).  The literal cases below are derived by hand from the arithmetic of the plan call;
tests/golden/saopd_forms.npz (tests/golden/gen/make_golden_saopd_forms.py) pins the two names and every derived size of
each of its queries, or the error the sizes get; tests/test_gpu_forms_reached.py compares the answers with what plans record."""
import os

import numpy as np
import pytest

from rl_agents_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("MP_SAOPD_MODEL", "MP_SAOPD_QUEUE", "MP_SAOPD_LANE_SCRATCH", "MP_SAOPD_PAR_BACKUP", "MP_SAOPD_CSR", "MP_SAOPD_PRUNE_ROWS",
         "MP_SAOPD_LDS", "MP_SAOPD_DICT", "MP_SAOPD_QUEUE_LIMIT_MB", "MP_SAOPD_ORDER")


@pytest.fixture(scope="module")
def forms():
    return np.load(os.path.join(REPO, "tests", "golden", "saopd_forms.npz"))


def _set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in knobs.split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv(k, v)


def choose(monkeypatch, knobs="", n=5, S=118, A=4, budget=120, n_nodes=0, have_cost=0, device_arrays=0):
    """-> (name, fallback, {field: value}) for fresh planners on 256 CUs and host arrays unless said otherwise; kept planners
    hold rows and a queue of the sizes a first plan of budget 120 gives them"""
    _set_knobs(monkeypatch, knobs)
    cap, qcap = (0, 0) if n_nodes == 0 else (n_nodes + n_nodes // 2, 4096)
    name, fallback, out = native.saopd_choose_form([n, S, A, budget, n_nodes, cap, qcap, have_cost, device_arrays, 256])
    return name, fallback, dict(zip(native.SAOPD_FORM_FIELDS, out.tolist()))


# ---- the cases derived by hand -------------------------------------------------------------------------------------------------
def test_dictionaries_up_to_117_states(monkeypatch):
    """5 KiB hold 32 B, 40 B per state and the depth tables of 24 B per entry: 117 states leave 408 B = 17 entries, 118 leave 15 --
    fewer than the 16 the form needs."""
    name, _, out = choose(monkeypatch, S=117)
    assert name == "saopd_wave_dict" and out["tab_lds"] == 17 and out["lds"] == 5120
    name, _, out = choose(monkeypatch, S=118)
    assert name == "saopd_wave_lds" and out["lds"] == 1312 + 16 + 121 * 36 + 118 * 20 + 4096 * 4 == 24428
    assert choose(monkeypatch, "MP_SAOPD_LDS=0", S=118)[0] == "saopd_wave"
    assert choose(monkeypatch, "MP_SAOPD_DICT=1 MP_SAOPD_LDS=0", S=118)[0] == "saopd_wave"      # the knob cannot force the form


def test_dictionaries_need_sixteen_depth_entries(monkeypatch):
    assert choose(monkeypatch, S=117, budget=48)[0] == "saopd_wave_lds"       # K + 3 = 15
    assert choose(monkeypatch, S=117, budget=52)[0] == "saopd_wave_dict"      # K + 3 = 16


def test_arena_in_lds_for_one_planner_per_cu_and_host_arrays(monkeypatch):
    assert choose(monkeypatch, n=256)[0] == "saopd_wave_lds"
    assert choose(monkeypatch, n=257)[0] == "saopd_wave"
    name, _, out = choose(monkeypatch, device_arrays=1)
    assert name == "saopd_wave" and out["sticky"] == 1
    assert choose(monkeypatch)[2]["sticky"] == 0


def test_asking_for_the_arena_in_lds_falls_back_on_the_dictionaries(monkeypatch):
    name, fallback, _ = choose(monkeypatch, "MP_SAOPD_LDS=1", S=117)
    assert (name, fallback) == ("saopd_wave_lds", "saopd_wave_dict")
    name, fallback, _ = choose(monkeypatch, S=118)
    assert (name, fallback) == ("saopd_wave_lds", "saopd_wave")
    name, fallback, _ = choose(monkeypatch, S=117)
    assert (name, fallback) == ("saopd_wave_dict", "saopd_wave_dict")


def test_dispatch_order_beyond_32_planners_per_cu_with_costs(monkeypatch):
    assert choose(monkeypatch, n=8193, have_cost=1)[0].endswith("_ordered")
    assert not choose(monkeypatch, n=8192, have_cost=1)[0].endswith("_ordered")
    assert not choose(monkeypatch, n=8193, have_cost=0)[0].endswith("_ordered")
    name, fallback, out = choose(monkeypatch, "MP_SAOPD_ORDER=1", n=5, have_cost=1)
    assert name == "saopd_wave_lds_ordered" and fallback == "saopd_wave_ordered" and out["ordered"] == 1
    name, _, out = choose(monkeypatch, "MP_SAOPD_ORDER=1", n=5, have_cost=0)
    assert name == "saopd_wave_lds" and out["ordered"] == 0
    assert not choose(monkeypatch, "MP_SAOPD_ORDER=0", n=8193, have_cost=1)[0].endswith("_ordered")


def test_one_planner_per_lane(monkeypatch):
    name, fallback, out = choose(monkeypatch, A=65)
    assert (name, fallback, out["wave"]) == ("saopd_lane", "saopd_lane", 0)
    name, fallback, out = choose(monkeypatch, "MP_SAOPD_MODEL=lane", A=4)
    assert (name, fallback, out["wave"]) == ("saopd_lane", "saopd_lane", 0)
    assert choose(monkeypatch, "MP_SAOPD_MODEL=lane MP_SAOPD_ORDER=1", A=4, have_cost=1)[0] == "saopd_lane"
    assert choose(monkeypatch, A=64)[2]["wave"] == 1


def test_lane_kernel_holds_every_depth_entry_in_lds(monkeypatch):
    """24 B per entry and 512 B: 2 709 entries are 65 528 B, one more passes 64 KiB; the wave kernels keep 2 560 in LDS."""
    name, _, out = choose(monkeypatch, A=65, budget=65 * 2706)
    assert name == "saopd_lane" and out["tab_plain"] == 2709 and out["lds"] == 24 * 2709 + 512 == 65528
    with pytest.raises(native.NativeError) as e:
        choose(monkeypatch, A=65, budget=65 * 2707)
    assert e.value.code == native.ERR_ARG and "of LDS tables" in str(e.value)
    with pytest.raises(native.NativeError) as e:
        choose(monkeypatch, "MP_SAOPD_MODEL=lane", A=4, budget=4 * 2707)
    assert e.value.code == native.ERR_ARG and "of LDS tables" in str(e.value)
    _, _, out = choose(monkeypatch, A=4, budget=65 * 2707)
    assert out["tab_plain"] == 2560 and out["K"] == 65 * 2707 // 4


def test_budget_beyond_the_depth_field(monkeypatch):
    assert choose(monkeypatch, S=3, budget=4 * (0x00ffffff - 2))[2]["K"] == 0x00ffffff - 2
    with pytest.raises(native.NativeError) as e:
        choose(monkeypatch, S=3, budget=4 * (0x00ffffff - 1))
    assert e.value.code == native.ERR_ARG and "budget too large" in str(e.value)


def test_queue_smaller_than_a_plan(monkeypatch):
    """MP_SAOPD_QUEUE rounds up to a power of two: 128 entries hold the 121 nodes of a plan, 64 do not."""
    _, _, out = choose(monkeypatch, "MP_SAOPD_QUEUE=100")
    assert out["qcap"] == 128 and out["lds_qcap"] == 128 and out["scap_global"] == 2
    with pytest.raises(native.NativeError) as e:
        choose(monkeypatch, "MP_SAOPD_QUEUE=64")
    assert e.value.code == native.ERR_ARG and "queue of 64 entries is smaller than the 121 nodes" in str(e.value)
    assert choose(monkeypatch)[2]["qcap"] == 4096
    assert choose(monkeypatch, budget=516)[2]["qcap"] == 32768            # 32 (1 + 516) = 16 544 entries


def test_par_backup_csr_and_prune_rows(monkeypatch):
    assert choose(monkeypatch)[2]["par_backup"] == 1 and choose(monkeypatch, n_nodes=121)[2]["par_backup"] == 0
    assert choose(monkeypatch, "MP_SAOPD_PAR_BACKUP=0")[2]["par_backup"] == 0
    assert choose(monkeypatch, "MP_SAOPD_PAR_BACKUP=1", n_nodes=121)[2]["par_backup"] == 1
    assert choose(monkeypatch)[2]["csr_old"] == 1
    assert choose(monkeypatch, "MP_SAOPD_CSR=0")[2]["csr_old"] == 0
    assert choose(monkeypatch, "MP_SAOPD_CSR=1")[2]["csr_old"] == 2 and choose(monkeypatch, "MP_SAOPD_CSR=x")[2]["csr_old"] == 2
    assert choose(monkeypatch)[2]["prune_rows"] == 256
    for value, rows in (("-5", 0), ("0", 0), ("7", 7), ("256", 256), ("257", 256), ("100000", 256)):
        assert choose(monkeypatch, "MP_SAOPD_PRUNE_ROWS=" + value)[2]["prune_rows"] == rows


def test_rows_and_their_growth(monkeypatch):
    """A fresh plan of budget 120 makes 121 rows and allocates half as many again; a kept planner grows when they run out."""
    out = choose(monkeypatch)[2]
    assert (out["K"], out["need"], out["cap"], out["lds_rows"]) == (30, 121, 181, 121)
    out = choose(monkeypatch, n_nodes=60)[2]            # 60 rows kept in 90: 181 needed
    assert (out["need"], out["cap"]) == (181, 181 + 90)
    _set_knobs(monkeypatch, "")
    out = native.saopd_choose_form([5, 118, 4, 120, 60, 181, 4096, 1, 0, 256])[2]
    assert out[native.SAOPD_FORM_FIELDS.index("cap")] == 181


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def test_saopd_forms_match_the_fixture(forms, monkeypatch):
    """Every query of the fixture gets the recorded names and sizes, or the recorded error."""
    bad = []
    for call, knobs, status, error, form, fallback, out in zip(forms["call"], forms["knobs"], forms["status"], forms["error"], forms["form"],
                                                              forms["fallback"], forms["out"]):
        _set_knobs(monkeypatch, str(knobs))
        try:
            got = native.saopd_choose_form(call)
            got = (0, True, got[0], got[1], got[2].tolist())
        except native.NativeError as e:
            got = (e.code, str(error) in str(e), "", "", [0] * len(native.SAOPD_FORM_FIELDS))
        want = (int(status), True, str(form), str(fallback), out.tolist())
        if got != want:
            bad.append((dict(zip(native.SAOPD_CALL_FIELDS, call.tolist())), str(knobs), want, got))
    assert not bad, "{} of {} queries differ, e.g. {}".format(len(bad), len(forms["call"]), bad[:3])


def test_saopd_forms_fixture_covers_every_form_and_error(forms):
    """The fixture reaches every name the library lists for the planner without "_retry", as a first launch and (but for the
    all-in-LDS form, which never is one) as a fallback, and every error of the choice."""
    names = {n for n in native.kernel_form_names() if n.startswith("saopd_") and not n.endswith("_retry")}
    assert len(names) == 7
    assert set(forms["form"].tolist()) == names | {""}
    assert set(forms["fallback"].tolist()) == {n for n in names if "_lds" not in n} | {""}
    assert set(forms["status"].tolist()) == {0, native.ERR_ARG}
    assert set(forms["error"].tolist()) == {"", "budget too large", "queue of", "of LDS tables"}
    assert len(set(forms["knobs"].tolist())) > 50 and len(forms["call"]) > 5000


def test_saopd_forms_read_the_knobs_at_each_call(monkeypatch):
    """The knobs are read per query: the same call changes form as they change, and changes back."""
    assert choose(monkeypatch, S=100)[0] == "saopd_wave_dict"
    assert choose(monkeypatch, "MP_SAOPD_DICT=0", S=100)[0] == "saopd_wave_lds"
    assert choose(monkeypatch, "MP_SAOPD_DICT=0 MP_SAOPD_LDS=0", S=100)[0] == "saopd_wave"
    assert choose(monkeypatch, "MP_SAOPD_MODEL=lane", S=100)[0] == "saopd_lane"
    assert choose(monkeypatch, "MP_SAOPD_LDS=1", S=100)[0] == "saopd_wave_lds"
    assert choose(monkeypatch, S=100)[0] == "saopd_wave_dict"


def test_saopd_choose_form_refuses_bad_sizes(monkeypatch):
    _set_knobs(monkeypatch, "")
    for bad in ([0, 100, 4, 120, 0, 0, 0, 0, 0, 256], [5, 100, 0, 120, 0, 0, 0, 0, 0, 256], [5, 100, 4, -1, 0, 0, 0, 0, 0, 256]):
        with pytest.raises(native.NativeError) as e:
            native.saopd_choose_form(bad)
        assert e.value.code == native.ERR_ARG
