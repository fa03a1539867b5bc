"""The inputs on which KL-OLOP's bound is held against the reference function itself (tests/golden/kl_bound.npz), built
deterministically: the golden's generator and the tests both call :func:`lattice` and compare checksums.

``kl_upper_bound(cumulative_reward, count, threshold)`` (utils.py:123-203) is a Newton iteration with discontinuous decisions
(the stop test at 1e-2, the clamps into [mu, 1]) and one branch that only a Python ``ZeroDivisionError`` reaches; the points
are the ones at which a planner's episodes put it: small counts with every integer sum, sums one ulp from 0 and from the
count, the thresholds ``4*log(t)`` / ``2*log(t)`` of the configs and the degenerate ones (0, tiny, huge, inf, NaN).
"""
import hashlib
import math

import numpy as np

ULP_BELOW_ONE = 1.0 - 2.0 ** -53            # the largest double below 1: (mu + 1) / 2 rounds to 1.0
COUNTS = list(range(1, 41)) + [55, 64, 100, 1000, 10 ** 6]
FRACTIONS = (5e-324, 2.2250738585072014e-308, 1e-17, .1, .3, .5, .7, .99, ULP_BELOW_ONE)
# 4*log(t) for t in 1 (= 0), 2, 3, 5, 8, 13, 21, 34, 55, 60 and 2*log(t) for t in 2, 7, 55, written out: the inputs, and with them
# the checksum, must not follow the last bit of whichever log evaluates them
LOG_THRESHOLDS = ("0x1.62e42fefa39efp+1", "0x1.193ea7aad030bp+2", "0x1.9c041f7ed8d33p+2", "0x1.0a2b23f3bab73p+3",
                  "0x1.485042b318c51p+3", "0x1.85b2e946faeb1p+3", "0x1.c35fc81b90df6p+3", "0x1.0078259bafef3p+4",
                  "0x1.0609bdc65328bp+4", "0x1.62e42fefa39efp+0", "0x1.f2272ae325a57p+1", "0x1.0078259bafef3p+3")
THRESHOLDS = sorted({0.0, 1e-300, 1e-9, 1.0, 1e6, math.inf} | {float.fromhex(h) for h in LOG_THRESHOLDS}) + [math.nan]


def lattice():
    """dict(total, count, threshold: the triples of kl_upper_bound; p, q: the pairs of bernoulli_kullback_leibler)."""
    rs = np.random.default_rng(7)
    total, count, threshold = [], [], []
    for t in THRESHOLDS:                       # a node never visited: the bound is 1 whatever the threshold
        total.append(0.0)
        count.append(0)
        threshold.append(t)
    for c in COUNTS:
        sums = set()
        for k in range(41):
            if c > 40:
                sums.add(float(k * (c // 40)))
            elif k <= c:
                sums.add(float(k))
        for u in FRACTIONS:
            sums.add(min(c * u, float(c)))
        sums.add(float(np.nextafter(float(c), 0.0)))
        for u in rs.random(6):
            sums.add(float(c * u))
        for s in sorted(sums):
            for t in THRESHOLDS:
                total.append(s)
                count.append(c)
                threshold.append(t)
    # pairs: p in [0, 1] and q each at 0, 1, one ulp from either; q at and beyond 1 (the infinite tail), q = x - eps below 0
    # as the finite difference at x = 0 passes it; then seeded pairs inside the unit square
    edge_p = [0.0, 5e-324, 2.2250738585072014e-308, 1e-17, .1, .3, .5, .7, .99, ULP_BELOW_ONE, 1.0]
    edge_q = edge_p + [float(np.nextafter(1.0, 2.0)), 1.5, 2.0, math.inf, -1e-2, 1.0 - 1e-2, 0.99 - 1e-2]
    p = [a for a in edge_p for _ in edge_q]
    q = [b for _ in edge_p for b in edge_q]
    rp = np.random.default_rng(11)
    u, v = rp.random(3000), rp.random(3000)
    v[:500] = u[:500] * (1 + 1e-3 * (rp.random(500) - 0.5))         # q close to p: the two logs nearly cancel
    v[500:700] = u[500:700]                                        # q == p: 0
    return dict(total=np.asarray(total, np.float64), count=np.asarray(count, np.int32),
                threshold=np.asarray(threshold, np.float64), p=np.concatenate([np.asarray(p, np.float64), u]),
                q=np.concatenate([np.asarray(q, np.float64), np.minimum(v, ULP_BELOW_ONE)]))


def checksum(lat):
    """sha256 over the bytes of the five arrays (NaN thresholds are the one quiet NaN of ``math.nan``)."""
    h = hashlib.sha256()
    for k in ("total", "count", "threshold", "p", "q"):
        a = np.ascontiguousarray(lat[k])
        h.update(k.encode() + str(a.dtype).encode() + a.tobytes())
    return h.hexdigest()
