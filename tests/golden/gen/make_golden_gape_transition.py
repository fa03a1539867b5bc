#!/usr/bin/env python3
"""Golden vectors for MDP-GapE's transition bound alone: the UNMODIFIED reference
``rl_agents.utils.max_expectation_under_constraint`` on a lattice of problems.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_gape_transition.py      (build container only)

-> tests/golden/gape_transition.npz: for K in {1, 2, 3, 5, 32} the inputs ``f<K>``, ``q<K>`` [n, K] and ``c<K>`` [n], the
reference's ``p<K>`` [n, K], its Newton ``iterations<K>``, the ``decisions<K>`` it took (the KT_* bits of
tests/gape_stoch_restatement.py) and ``flag<K>``; and ``f_hand`` ... ``flag_hand``, the same for a few hand-made points of width 4
(``hand_made``: the ``beta == 0`` branches).  Inputs and outputs only.

The lattice: ``q`` with no, some and only zeros (counts over their sum, as a chance node's frequencies); ``f`` random, with
ties at the maximum among the zero-probability entries and among the others, and with every ``f_p`` inside and just outside
numpy's ``isclose`` allowance of the first; both signs of ``f`` (the lower solve takes ``-l_next``); ``c`` in {0, 1e-3, 0.1, 2}.
Every kind of ``q`` meets every kind of ``f`` three times at each ``c`` > 0.  ``c == 0`` has one point per kind of ``f``: there
``theta`` has its root at infinity, the reference's Newton iteration walks out along a flat tail until its own step falls below
eps, and where it stops hangs on the cancellation in ``theta`` -- the reference's own ``p_star`` moves by up to 4e-8 under the
jitter below at most such points that take Newton steps (a planner's ``c`` is 0 only for ``time == 1``).  They are in the file for the branches
they take; few, so that the flagged share stays what it is on the rest of the lattice.

The trace is the reference's own: the restatement runs on the same inputs, must return the reference's ``p_star`` bit for bit,
and the calls the reference made of its ``theta_func`` must number the restatement's iterations (plus the one at ``f_star``).

``flag``: the reference's OWN ``p_star`` moves by more than 1e-13 (or changes shape of branch: another NaN pattern) when every
``np.log`` / ``np.exp`` inside ``rl_agents/utils.py`` is moved by up to 2 ulp -- a point that hangs on the last bits of libm,
which no device can be held to.  The script asserts that at most 5 % of the points carry it.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401
from make_golden import np  # noqa: E402

np.infty = np.inf
from rl_agents import utils as ref_utils  # noqa: E402

from tests import gape_stoch_restatement as gs  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "gape_transition.npz"))
WIDTHS = (1, 2, 3, 5, 32)
THRESHOLDS = (0.0, 1e-3, 0.1, 2.0)
FLAG_MOVE, FLAG_CAP, ULPS = 1e-13, 0.05, 2


class JitteredNumpy(object):
    """numpy with ``log`` and ``exp`` moved by up to ULPS units in the last place, seeded; everything else is numpy's."""

    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))

    def __getattr__(self, name):
        return getattr(np, name)

    def moved(self, y):
        y = np.asarray(y, np.float64)
        k = self.rng.integers(-ULPS, ULPS + 1, size=y.shape)
        out = y.copy()
        for _ in range(ULPS):
            out = np.where(np.isfinite(y) & (k > 0), np.nextafter(out, np.inf), out)
            out = np.where(np.isfinite(y) & (k < 0), np.nextafter(out, -np.inf), out)
            k = k - np.sign(k)
        return out if out.ndim else np.float64(out)

    def log(self, x):
        with np.errstate(all="ignore"):
            return self.moved(np.log(x))

    def exp(self, x):
        with np.errstate(all="ignore"):
            return self.moved(np.exp(x))


def reference(f, q, c):
    """(p_star, calls of theta_func) of the unmodified reference."""
    calls = [0]
    theta0 = ref_utils.theta_func

    def counted(*args, **kwargs):
        calls[0] += 1
        return theta0(*args, **kwargs)

    ref_utils.theta_func = counted
    try:
        with np.errstate(all="ignore"):
            p = ref_utils.max_expectation_under_constraint(f.copy(), q.copy(), c)
    finally:
        ref_utils.theta_func = theta0
    return np.asarray(p, np.float64), calls[0]


def reference_jittered(f, q, c, seed):
    ref_utils.np = JitteredNumpy(seed)
    try:
        with np.errstate(all="ignore"):
            return np.asarray(ref_utils.max_expectation_under_constraint(f.copy(), q.copy(), c), np.float64)
    finally:
        ref_utils.np = np


def lattice(K, rng):
    points = []
    q_kinds = ("none", "some", "all") if K > 1 else ("none", "all")
    f_kinds = ("random", "tie_zero", "tie_plus", "close_in", "close_out")
    for q_kind in q_kinds:
        for i_f, f_kind in enumerate(f_kinds):
            for c in THRESHOLDS:
                # c == 0 asks for a root at infinity (see the module docstring): one point per kind of f, the kinds of q in turn
                if c == 0 and q_kind != q_kinds[i_f % len(q_kinds)]:
                    continue
                for rep in range(1 if c == 0 else 3):
                    counts = rng.integers(1, 6, size=K).astype(np.float64)
                    if q_kind == "some":
                        zeros = rng.permutation(K)[:rng.integers(1, K)]
                        counts[zeros] = 0
                    q = counts / counts.sum() if q_kind != "all" else np.zeros(K)
                    plus = np.flatnonzero(q > 0) if q_kind != "all" else np.arange(K)
                    zero = np.flatnonzero(q == 0) if q_kind != "all" else np.zeros(0, np.int64)
                    f = rng.uniform(0.0, 3.0, size=K)
                    if f_kind == "tie_zero" and len(zero):
                        f[zero[:2]] = 3.5                                   # the maximum, once or twice, where q is 0
                        if len(zero) > 2:
                            f[zero[2]] = f[zero[-1]]
                    elif f_kind == "tie_plus":
                        f[plus[:2]] = 3.5                                   # the maximum, once or twice, where q > 0
                        if len(plus) > 3:
                            f[plus[3]] = f[plus[2]]                         # and a tie below it
                    elif f_kind in ("close_in", "close_out"):
                        base = rng.uniform(0.5, 3.0)
                        f[plus] = base + rng.uniform(-1.0, 1.0, size=len(plus)) * 0.9 * (1e-8 + 1e-5 * base)
                        f[plus[0]] = base
                        if f_kind == "close_out" and len(plus) > 1:
                            f[plus[-1]] = base + (1.0 if rep else -1.0) * 1.001 * (1e-8 + 1e-5 * base) + (1e-12 if rep else -1e-12)
                    if rep % 2:
                        f = -f                                              # the lower solve's sign
                    points.append((f, q, c))
    return points


HAND_WIDTH = 4


def hand_made():
    """Points of width 4 for the branches no lattice point takes (stored as ``f_hand`` ...).  ``beta == 0`` without the uniform
    fallback: a threshold so large that ``exp(theta_star)`` underflows, z == 1 and nothing is left for the entries of positive
    probability (the zero-probability maximum alone, and tied).  ``beta == 0`` WITH the fallback: values of the order 1e13 with a
    large threshold, where the Newton iterate is pulled back to ``0.9 * a + 0.1 * x`` until it rounds onto ``a = f_star`` itself,
    ``1 / (lambda - f_p)`` is infinite at the maximum and ``beta`` is 1 / inf (found by a seeded search over the restatement).
    The final clamp (an iterate below ``a`` when the loop ends) is not among them: the pull-back keeps every iterate at or above
    ``a`` except through rounding, and that search (400 000 points, magnitudes 1 .. 1e13) met none."""
    counted = [
        ([0.5, 2.0, 2.0, -1.0], [1.0, 0.0, 0.0, 1.0], 800.0),
        ([1.0, 2.0, 0.0, 0.5], [1.0, 0.0, 0.0, 0.0], 1000.0),
        ([-1.0, -2.0, -0.25, -0.5], [2.0, 1.0, 0.0, 1.0], 900.0),
        ([-9986864832883.174, -2247891648369.207, 9251260831437.238, 5274838508767.818], [2.0, 0.0, 1.0, 2.0], 563.8850732056594),
        ([9746411538001.826, 2300932282919.419, -9033491071411.03, -6368499225201.751], [3.0, 3.0, 2.0, 1.0], 882.5023038867718),
        ([-2235549737613.287, 9833371099709.492, -7860010129660.973, -3026120038998.068], [0.0, 3.0, 0.0, 3.0], 239.00124459934906),
        ([8926644973041.58, 920713836765.7585, -6829424129929.2, -2595583348060.029], [1.0, 3.0, 3.0, 0.0], 98.25588890800601),
        ([8806122527904.406, -3284283619674.346, -333791015968.3877, 9186768925596.914], [1.0, 3.0, 1.0, 3.0], 41.34371845747007),
        ([-5896738245915.51, 78755061733.34435, 4957432381534.781, 9032925071855.54], [2.0, 3.0, 0.0, 3.0], 215.43210166332514),
    ]
    return [(np.asarray(f, np.float64), np.asarray(n, np.float64) / np.sum(n), c) for f, n, c in counted]


def main():
    store, total, flagged = {}, 0, 0
    for K in WIDTHS + ("_hand",):
        rng = np.random.Generator(np.random.PCG64(1000 + K)) if K != "_hand" else None
        rows = dict(f=[], q=[], c=[], p=[], iterations=[], decisions=[], flag=[])
        for f, q, c in (lattice(K, rng) if K != "_hand" else hand_made()):
            p_ref, calls = reference(f, q, c)
            p, its, mask = gs.max_expectation(f, q, c)
            assert np.array_equal(p, p_ref, equal_nan=True), (K, f, q, c, p, p_ref)
            assert calls == its + bool(mask & gs.KT_FSTAR_ABOVE), (K, f, q, c, calls, its, mask)
            flag = False
            for seed in (1, 2):
                moved = reference_jittered(f, q, c, seed)
                same_kind = np.array_equal(np.isnan(moved), np.isnan(p_ref))
                flag |= not same_kind or bool(np.nanmax(np.abs(moved - p_ref), initial=0.0) > FLAG_MOVE)
            for k, v in zip(("f", "q", "c", "p", "iterations", "decisions", "flag"), (f, q, c, p_ref, its, mask, flag)):
                rows[k].append(v)
        n = len(rows["c"])
        total += n
        flagged += int(np.sum(rows["flag"]))
        dt = dict(iterations=np.int32, decisions=np.int32, flag=bool)
        for k, v in rows.items():
            store["{}{}".format(k, K)] = np.asarray(v, dt.get(k, np.float64))
        masks = np.asarray(rows["decisions"])
        print("K {:>5}: {:4d} points, flagged {:3d}, iterations up to {:3d}, branches {}".format(
            K, n, int(np.sum(rows["flag"])), int(np.max(rows["iterations"])),
            {b: int(np.sum((masks & b) != 0)) for b in (1, 2, 4, 8, 16, 32, 64, 128, 256)}))
    assert flagged <= FLAG_CAP * total, (flagged, total)
    hand = store["decisions_hand"][~store["flag_hand"]]
    assert (hand & gs.KT_BETA_ZERO).all() and (hand & gs.KT_BETA_UNIFORM).any() and not (hand & gs.KT_BETA_UNIFORM).all(), hand
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, total, "points,", flagged, "flagged,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
