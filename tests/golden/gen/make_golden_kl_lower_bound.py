#!/usr/bin/env python3
"""Golden vectors for MDP-GapE's lower bound: the UNMODIFIED reference ``rl_agents.utils.kl_upper_bound(..., lower=True)``
(with its ``newton_iteration``) on a grid of (cumulative reward, count, threshold).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_kl_lower_bound.py      (build container only)

-> tests/golden/kl_lower_bound.npz: the inputs ``total``, ``count``, ``threshold`` and, per point, what the reference returned
(``bound``), the Newton iterations it ran and the decisions it took (the bit mask of ``mp_selftest_olop_bound``).  Nothing of
the reference is copied: inputs and its outputs only.

The iterations and the finite difference are OBSERVED: ``newton_iteration`` is called through a wrapper that counts the calls
of the derivative it was handed and notes a ZeroDivisionError passing through.  The clamps cannot be seen from outside the
function; they are those of the test-side restatement (tests/gape_restatement.py), which is first held to the reference's
value bit for bit and to the observed iterations and finite differences at every point.

The grid: mu in {0, 1, tiny, near 1, interior} as exact and as inexact quotients, counts 1 .. 200, and thresholds from both
threshold strings of the reference's configs (the default of mdp_gape.py:33-35 and "1*np.log(time)").
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (puts the stubs, the reference and this repository on sys.path)
from make_golden import np  # noqa: E402

np.infty = np.inf
from rl_agents import utils as ref_utils  # noqa: E402

from tests import gape_restatement as gr  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "kl_lower_bound.npz"))


def grid():
    counts = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 200] + list(range(4, 200, 17))
    mus = [0.0, 1.0, 5e-324, 1e-300, 1e-12, 1e-3, 1 - 1e-12, 1 - 2.0 ** -53, 0.999, 0.1, 0.25, 1 / 3, 0.5, 0.7, 0.9]
    thresholds = []
    for count in (1, 2, 7, 50, 200):
        for horizon, actions, confidence in ((2, 3, 0.9), (9, 5, 0.9), (3, 70, 0.5)):
            thresholds.append(float(eval(gr.DEFAULT_THRESHOLD, {"np": np}, dict(count=count, horizon=horizon, actions=actions,
                                                                                 confidence=confidence))))
    thresholds += [float(1 * np.log(time)) for time in (1, 2, 8, 55, 400)]
    total, cnt, thr = [], [], []
    for c in counts:
        for mu in mus:
            for t in thresholds[::2] if c % 2 else thresholds[1::2]:
                total.append(mu * c)
                cnt.append(c)
                thr.append(t)
    return np.asarray(total, np.float64), np.asarray(cnt, np.int32), np.asarray(thr, np.float64)


def main():
    total, count, threshold = grid()
    seen = {}
    newton0 = ref_utils.newton_iteration

    def newton(f, df, eps, **kw):
        def counted(x):
            seen["iterations"] += 1
            try:
                return df(x)
            except ZeroDivisionError:
                seen["fd"] = True
                raise
        return newton0(f, counted, eps, **kw)

    ref_utils.newton_iteration = newton
    warnings.simplefilter("ignore")
    bound, iterations, decisions = [], [], []
    try:
        with np.errstate(all="ignore"):
            for s, c, t in zip(total, count, threshold):
                seen.update(iterations=0, fd=False)
                ref = float(ref_utils.kl_upper_bound(float(s), int(c), float(t), lower=True))
                mine, its, mask = gr.kl_bound_traced(float(s), int(c), float(t), lower=True)
                assert np.array_equal(ref, float(mine), equal_nan=True), (s, c, t, ref, mine)
                assert its == seen["iterations"] and bool(mask & 4) == seen["fd"], (s, c, t, its, seen)
                bound.append(ref); iterations.append(its); decisions.append(mask)
    finally:
        ref_utils.newton_iteration = newton0
    np.savez_compressed(OUT, total=total, count=count, threshold=threshold, bound=np.asarray(bound, np.float64),
                        iterations=np.asarray(iterations, np.int32), decisions=np.asarray(decisions, np.int32))
    print("wrote", OUT, len(bound), "points;", int(np.isnan(bound).sum()), "NaN; masks", sorted(set(decisions)),
          "iterations up to", max(iterations), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
