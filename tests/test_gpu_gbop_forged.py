"""Forged draws for GBOP on the device: the four kinds of draw a plan makes, put where no seed puts them (tests/gbop_cases.py
builds the cases on tests/forge.py and tests/forged_clone_cases.py; tests/test_gbop_cases_host.py ties each to numpy and
asserts what its restatement meets).

  the ties of random_argmax      k = 3, 6, 7, 70, 150 listed actions, every forge.TIE_CASES record that fits behind the seed word:
                                 0, 1 and 2 rejected words, a word on the edge of the bounded draw, a buffered word; the second
                                 step's tie and get_plan's start on whatever half the first left; tables and one-hot dense models
  the clone's draw               forged_clone_cases.clone_twins: the row search on and one step below every threshold, dense rows of
                                 150 (b = 0, 62, 63, 64, 127, 148) and sparse rows of 1, 3, 4, 5, at the first and the second step;
                                 the clone seeded with 0, 1 and 2^30 - 1
  get_plan's weighted choice     u on and one step below entries of the uniform cdf of K = 2, 3, 4, 32 placeholders, u = 0 and
                                 u = 1 - 2^-53; the choice of a tried action through slot (idx + c_m) % K

Compared with the restatement driven by forge.LoggingStream over the same record, as the sweep compares: status, plan with its
key, the generator record after the plan, env_steps, pops exactly; the exported graph within BOUND_TOL / (1 - gamma)."""
import numpy as np
import pytest

from rl_agents_amd import native
from tests import gbop_cases as gc
from tests.test_gpu_gbop_shapes import run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """Every case of this file with the restatement's answer, computed once."""
    return {name: gc.get_case(name) for family in ("tie", "clone", "choice") for name in gc.FAMILIES[family][0]}


@pytest.mark.parametrize("name", gc.TIE_NAMES)
def test_gbop_tie_draws(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    if gc.set_aside(name):
        return      # margin-fragile in the restatement: counted in tests/test_gbop_cases_host.py
    run_case(ctx, monkeypatch, case, ref)


@pytest.mark.parametrize("name", tuple(gc.CLONE))
def test_gbop_clone_draw_on_and_below_every_threshold(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    assert not gc.set_aside(name)
    _, exports, _ = run_case(ctx, monkeypatch, case, ref)
    K = case["K"]
    for twin in case["twins"]:
        want = gc.clone_want(case, twin)
        if want is None:
            continue
        lst = exports[twin["root"]]
        node = int(np.nonzero(lst["state"] == twin["state"])[0][0])
        a = twin["action"]
        # one child stands for a state: the dict order is the slots 1 .. K - 1, 0
        assert lst["c_count"][node, a] == 1 and lst["k_state"][node, a, K - 1] == want, (twin["root"], twin["b"], twin["twin"])
        assert (lst["k_state"][node, a, :K - 1] < 0).all()


@pytest.mark.parametrize("name", gc.CHOICE_NAMES)
def test_gbop_weighted_choice_on_the_boundary(ctx, monkeypatch, refs, name):
    case, ref = refs[name]
    assert not gc.set_aside(name)
    outs, _, _ = run_case(ctx, monkeypatch, case, ref)
    for i, want in enumerate(case["want"]):
        assert int(outs[0]["plans"].reshape(-1)[i]) == want["action"], i
        assert "placeholder_{}".format(-1 - int(outs[0]["key"][i])) == want["key"], i


def test_gbop_weighted_choice_of_a_tried_action(ctx, monkeypatch, refs):
    case, ref = refs["choice_tried"]
    assert not gc.set_aside("choice_tried") and ref["choice_margin"] > gc.MARGIN
    outs, exports, _ = run_case(ctx, monkeypatch, case, ref)
    assert (outs[0]["key"] >= 0).all() and (outs[0]["plan_len"] == 2).all()
