"""Pcg64W (csrc/pcg64.hpp): the PCG64 step on four 32-bit words, restated on Python integers (tests/pcg64_words_cases.py)
against state * MULT + inc (mod 2^128), against the output function on the 64-bit halves, and against numpy's own PCG64
streams.  The case list sets every carry of the increment chain to 0 and to 1 (c1 cannot be set: C1_NEVER); the same list runs through the header on the host
(tests/test_pcg64_words_host.py) and through the rollouts on the device (tests/test_gpu_uct_pcg_words.py).  No GPU."""
import random

import numpy as np
import pytest

from tests import pcg64_words_cases as pw


def test_the_case_list_sets_every_carry_both_ways():
    flags = {name: pw.words_step(s, i)[1] for name, s, i in pw.CASES}
    assert pw.C1_NEVER                               # (m0 + m1 < 2^32: column 1 cannot reach 2^64 -- no record sets c1)
    assert {flags[n]["c1"] for n in flags} == {0}
    for f in pw.FLAGS[1:]:
        assert {flags[n][f] for n in flags} == {0, 1}, f
        assert flags["{}=0".format(f)][f] == 0 and flags["{}=1".format(f)][f] == 1
    assert all(flags["all=1"][f] == 1 for f in pw.FLAGS[1:]) and all(flags["all=0"][f] == 0 for f in pw.FLAGS)
    # the last word: the sum exactly on 2^32 (with k2 = 1: only the carry takes it there), one below it, far beyond it
    for k2 in (0, 1):
        exact, below, far = (flags["w3_{}_k2={}".format(w, k2)] for w in ("exact", "below", "far"))
        assert exact["k2"] == below["k2"] == far["k2"] == k2
        assert exact["wrap3"] == 1 and below["wrap3"] == 0
    assert flags["w3_far_k2=1"]["wrap3"] == 1
    for name, s, i in pw.CASES:
        assert i & 1, name                           # (the device forces the bit when it loads a record)
        if name.startswith("w3_exact"):
            assert pw.words_step(s, i)[0] >> 96 == 0, name
        if name.startswith("w3_below"):
            assert pw.words_step(s, i)[0] >> 96 == pw.M32, name
    assert flags["ones"]["c1"] in (0, 1) and ("ones", pw.M128, pw.M128) in pw.CASES


def test_the_case_list_holds_the_rotations_0_31_32_63():
    for rot in (0, 31, 32, 63):
        for end in ("lo", "hi"):
            s, i = next((s, i) for name, s, i in pw.CASES if name == "rot{}_{}".format(rot, end))
            assert pw.step(s, i) >> 122 == rot


@pytest.mark.parametrize("name,state,inc", pw.CASES, ids=[c[0] for c in pw.CASES])
def test_step_and_output_on_the_cases(name, state, inc):
    new, _ = pw.words_step(state, inc)
    assert new == pw.step(state, inc)
    lo, hi = pw.words_output(new)
    assert (hi << 32) | lo == pw.output(new)
    lo, hi = pw.words_output(state)                  # (the output of the case itself: other rotations)
    assert (hi << 32) | lo == pw.output(state)


def test_step_and_output_on_random_records():
    g = random.Random(20240607)
    seen = {f: set() for f in pw.FLAGS[1:] + ("wrap3",)}
    rots = set()
    for _ in range(50000):
        s, i = g.getrandbits(128), g.getrandbits(128) | 1
        new, f = pw.words_step(s, i)
        assert new == pw.step(s, i)
        lo, hi = pw.words_output(new)
        assert (hi << 32) | lo == pw.output(new)
        rots.add(new >> 122)
        for k in seen:
            seen[k].add(f[k])
    assert all(v == {0, 1} for v in seen.values()) and rots == set(range(64))


def test_sparse_words_where_single_products_carry():
    """states and increments built from the words 0, 1, 2^31, 2^32 - 2 and 2^32 - 1: 5^8 records"""
    vals = (0, 1, 1 << 31, pw.M32 - 1, pw.M32)
    n = 0
    for idx in range(5 ** 8):
        d, w = idx, []
        for _ in range(8):
            w.append(vals[d % 5])
            d //= 5
        s = w[0] | (w[1] << 32) | (w[2] << 64) | (w[3] << 96)
        i = (w[4] | 1) | (w[5] << 32) | (w[6] << 64) | (w[7] << 96)
        new, _ = pw.words_step(s, i)
        assert new == pw.step(s, i)
        lo, hi = pw.words_output(new)
        assert (hi << 32) | lo == pw.output(new)
        n += 1
    assert n == 390625


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 63 + 11])
def test_against_numpy_streams(seed):
    bg = np.random.PCG64(np.random.SeedSequence(seed))
    st = bg.state["state"]
    state, inc = st["state"], st["inc"]
    want = bg.random_raw(2000)
    for k in range(2000):
        state, _ = pw.words_step(state, inc)
        lo, hi = pw.words_output(state)
        assert (hi << 32) | lo == int(want[k]), k
    assert state == bg.state["state"]["state"]


def test_numpy_streams_from_the_cases():
    """numpy's generator set to each case's state and increment: its next outputs are the word step's"""
    bg = np.random.PCG64(0)
    for name, state, inc in pw.CASES:
        st = bg.state
        st["state"] = {"state": state, "inc": inc}
        st["has_uint32"], st["uinteger"] = 0, 0
        bg.state = st
        want = bg.random_raw(3)
        for k in range(3):
            state, _ = pw.words_step(state, inc)
            lo, hi = pw.words_output(state)
            assert (hi << 32) | lo == int(want[k]), (name, k)


def test_record_of_steps_back():
    for name, state, inc in pw.CASES[:12]:
        for back in (0, 1, 2):
            rec = pw.record_of(state, inc, back)
            s = (rec[0] << 64) | rec[1]
            for _ in range(back):
                s = pw.step(s, inc)
            assert s == state and rec[2:] == [inc >> 64, inc & pw.M64, 0, 0], (name, back)
