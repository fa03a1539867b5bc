"""CPU tests of the UCT planner's choice of kernel form (mp_uct_choose_form: the function mp_uct_plan* calls, run on the host
alone).  tests/golden/uct_forms.npz (tests/golden/gen/make_golden_uct_forms.py) pins the form, the tree layout, the geometry
and the LDS bytes of every query, or the error its shape gets."""
import os

import numpy as np
import pytest

from rl_agents_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_LONE_WAVES", "MP_UCT_EACH", "MP_UCT_ROW", "MP_UCT_ROWS",
         "MP_UCT_ROW_WAVES", "MP_UCT_ROW_ROOTS", "MP_UCT_PATH", "MP_UCT_LANES", "MP_UCT_LDSR_WAVES", "MP_UCT_CART_REP",
         "MP_UCT_CART_WAVES")


@pytest.fixture(scope="module")
def forms():
    return np.load(os.path.join(REPO, "tests", "golden", "uct_forms.npz"))


def _set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in knobs.split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv(k, v)


def test_uct_forms_match_the_fixture(forms, monkeypatch):
    """Every query of the fixture gets the recorded form, layout, geometry and LDS bytes, or the recorded error."""
    bad = []
    for call, knobs, status, form, out in zip(forms["call"], forms["knobs"], forms["status"], forms["form"], forms["out"]):
        _set_knobs(monkeypatch, str(knobs))
        try:
            got = native.uct_choose_form(call)
            got = (0, got[0], got[1].tolist())
        except native.NativeError as e:
            got = (e.code, "", [0] * len(native.UCT_FORM_FIELDS))
        want = (int(status), str(form), out.tolist())
        if got != want:
            bad.append((dict(zip(native.UCT_CALL_FIELDS, call.tolist())), str(knobs), want, got))
    assert not bad, "{} of {} queries differ, e.g. {}".format(len(bad), len(forms["call"]), bad[:3])


def test_uct_forms_fixture_covers_every_form(forms):
    """The fixture reaches every form the chooser has, and errors."""
    assert set(forms["form"].tolist()) == {"", "uct_global", "uct_global_spill", "uct_ldsr", "uct_quad", "uct_lone",
                                           "uct_lone_mw", "uct_lone_each", "uct_row_each", "uct_row_shared", "uct_cartpole",
                                           "uct_policy"}
    assert set(forms["status"].tolist()) == {0, native.ERR_ARG}


def test_uct_forms_read_the_knobs_at_each_call(monkeypatch):
    """The knobs are read per call: the same query changes form as they change."""
    headline = [4096, 33, 30, 5, 10000, 1, 10000, 1, 1, 7, 0, 0, -1, 256]
    _set_knobs(monkeypatch, "")
    assert native.uct_choose_form(headline)[0] == "uct_row_shared"
    _set_knobs(monkeypatch, "MP_UCT_MODEL=ldsr")
    assert native.uct_choose_form(headline)[0] == "uct_ldsr"
    _set_knobs(monkeypatch, "MP_UCT_MODEL=global")
    assert native.uct_choose_form(headline)[0] == "uct_global"
    _set_knobs(monkeypatch, "")
    assert native.uct_choose_form(headline)[0] == "uct_row_shared"


def test_uct_forms_refuse_a_policy_over_more_than_eight_actions(monkeypatch):
    _set_knobs(monkeypatch, "")
    with pytest.raises(native.NativeError) as e:
        native.uct_choose_form([16, 33, 30, 11, 1000, 1, 1000, 1, 1, 3, 0, 1, -1, 256])
    assert e.value.code == native.ERR_ARG and "2..8" in str(e.value)
