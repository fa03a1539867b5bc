#!/usr/bin/env python3
"""The kernel form mp_saopd_plan chooses, pinned for tests/test_saopd_forms.py (host only: no GPU is needed or used).

    python3 tests/golden/gen/make_golden_saopd_forms.py

-> tests/golden/saopd_forms.npz, one row per query:
   call     int64 [N, 10]  the call's description (native.SAOPD_CALL_FIELDS)
   knobs    str   [N]      the MP_SAOPD_* knobs set for it, "NAME=value" joined by spaces ("" = none)
   status   int32 [N]      0, or the error code the plan returns for those sizes
   error    str   [N]      a phrase of the error's message ("" without one)
   form     str   [N]      the name of the first launch ("" on error)
   fallback str   [N]      the form a full backup queue falls back to ("" on error)
   out      int64 [N, 20]  native.SAOPD_FORM_FIELDS (zeros on error)
The queries: every edge of the thresholds on states, budget, batch size and the LDS sizes, fresh and kept planners, host and
device arrays, each knob alone, the knobs' interactions, and a seeded sample.  The fixture records what the library answers;
tests/test_saopd_forms.py holds the cases derived by hand, and the GPU tests compare the answers with what plans record.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, REPO)

from rl_agents_amd import native  # noqa: E402

KNOBS = ("MP_SAOPD_MODEL", "MP_SAOPD_QUEUE", "MP_SAOPD_LANE_SCRATCH", "MP_SAOPD_PAR_BACKUP", "MP_SAOPD_CSR", "MP_SAOPD_PRUNE_ROWS",
         "MP_SAOPD_LDS", "MP_SAOPD_DICT", "MP_SAOPD_QUEUE_LIMIT_MB", "MP_SAOPD_ORDER")
ERRORS = ("budget too large", "queue of", "of LDS tables")


def call(n=5, S=100, A=4, budget=120, n_nodes=0, cap=0, qcap=0, have_cost=0, device_arrays=0, cus=256):
    return (n, S, A, budget, n_nodes, cap, qcap, have_cost, device_arrays, cus)


ALONE = [("MP_SAOPD_MODEL", v) for v in ("lane", "l", "wave", "")] + \
        [("MP_SAOPD_QUEUE", v) for v in ("1", "100", "256", "4096", "5000", "1000000")] + \
        [("MP_SAOPD_LANE_SCRATCH", v) for v in ("-1", "0", "1", "63", "64", "1000")] + \
        [("MP_SAOPD_PAR_BACKUP", v) for v in ("0", "1", "2")] + [("MP_SAOPD_CSR", v) for v in ("0", "1", "2", "x")] + \
        [("MP_SAOPD_PRUNE_ROWS", v) for v in ("-5", "0", "1", "255", "256", "257", "100000")] + \
        [("MP_SAOPD_LDS", v) for v in ("0", "1", "2")] + [("MP_SAOPD_DICT", v) for v in ("0", "1", "2")] + \
        [("MP_SAOPD_QUEUE_LIMIT_MB", v) for v in ("0", "1", "64")] + [("MP_SAOPD_ORDER", v) for v in ("0", "1", "2")]

INTERACTIONS = [
    "MP_SAOPD_DICT=0 MP_SAOPD_LDS=0", "MP_SAOPD_DICT=1 MP_SAOPD_LDS=0", "MP_SAOPD_DICT=0 MP_SAOPD_LDS=1", "MP_SAOPD_DICT=1 MP_SAOPD_LDS=1",
    "MP_SAOPD_LDS=1 MP_SAOPD_QUEUE=256", "MP_SAOPD_LDS=1 MP_SAOPD_ORDER=1", "MP_SAOPD_ORDER=1 MP_SAOPD_QUEUE=256",
    "MP_SAOPD_MODEL=lane MP_SAOPD_QUEUE=256", "MP_SAOPD_MODEL=lane MP_SAOPD_LDS=1", "MP_SAOPD_MODEL=lane MP_SAOPD_DICT=1",
    "MP_SAOPD_MODEL=lane MP_SAOPD_ORDER=1", "MP_SAOPD_DICT=0 MP_SAOPD_LDS=0 MP_SAOPD_ORDER=1 MP_SAOPD_QUEUE=256",
    "MP_SAOPD_QUEUE=256 MP_SAOPD_LANE_SCRATCH=1", "MP_SAOPD_LDS=1 MP_SAOPD_LANE_SCRATCH=2", "MP_SAOPD_QUEUE=64 MP_SAOPD_LDS=1",
]


def lds_resident_rows(S, A, budget):
    """the most rows after the plan with which a fresh-sized arena still fits the all-in-LDS form (K = budget // A)"""
    k = budget // A
    tables = 3 * min(k + 3, 2560) * 8 + 512
    q = 4096
    while q < 2 * (1 + k * A) and q < (1 << 20):
        q <<= 1
    return (160 * 1024 - 1024 - (((tables + 15) & ~15) + 16 + S * 20 + q * 4)) // 36


def queries():
    """-> [(call, knobs)]"""
    q = []
    # the dictionaries' edge in states and in budget, host and device arrays, fresh and kept, batches around one planner per CU
    for S in (1, 3, 100, 116, 117, 118, 119, 127, 128, 1000, 10000):
        for budget in (0, 3, 8, 48, 51, 52, 120, 500, 1200):
            for n in (1, 5, 70, 256, 257):
                q += [(call(n=n, S=S, budget=budget, device_arrays=d), "") for d in (0, 1)]
            q += [(call(S=S, budget=budget, n_nodes=121, cap=181, qcap=4096, have_cost=1), k) for k in ("", "MP_SAOPD_LDS=1")]
    # compute units: one planner per CU and 32 per CU, with and without costs
    for cus in (256, 80, 304, 0):
        c = cus or 256
        for n in (c - 1, c, c + 1, 32 * c - 1, 32 * c, 32 * c + 1):
            for S in (100, 118):
                q += [(call(n=n, S=S, have_cost=h, cus=cus), k) for h in (0, 1) for k in ("", "MP_SAOPD_ORDER=1", "MP_SAOPD_ORDER=0")]
    # a kept planner grows out of the all-in-LDS form
    for S, A, budget in ((100, 4, 1200), (118, 4, 120), (118, 4, 500)):
        rows = lds_resident_rows(S, A, budget)
        per_plan = 1 + (budget // A) * A
        for need in (rows - 1, rows, rows + 1):
            kept = max(need - per_plan, 0)
            q += [(call(n=3, S=S, A=A, budget=budget, n_nodes=kept, cap=kept, qcap=4096, have_cost=1), k) for k in ("", "MP_SAOPD_LDS=1")]
    # row growth: with and without slack
    for cap in (0, 100, 121, 181, 182, 5000):
        for n_nodes in (0, 61, 121, 4000):
            if n_nodes <= cap:
                q += [(call(n_nodes=n_nodes, cap=cap, qcap=4096, budget=b), "") for b in (120, 500, 20000)]
    # the queue: its size by budget, a queue kept from an earlier plan, the knob against either
    for budget in (0, 120, 508, 512, 516, 2044, 2048, 40000):
        for qcap in (0, 256, 4096, 65536):
            q += [(call(budget=budget, qcap=qcap, n_nodes=0 if qcap == 0 else 121, cap=0 if qcap == 0 else 181), k)
                  for k in ("", "MP_SAOPD_QUEUE=256", "MP_SAOPD_QUEUE=100", "MP_SAOPD_QUEUE=256 MP_SAOPD_LDS=1")]
    # action counts: the mapping, the lane kernel's LDS tables at their limit, the wave kernels' 2 560 entries
    for A in (1, 2, 4, 63, 64, 65, 100):
        q += [(call(A=A, budget=b, n=n), k) for b in (0, A - 1, A, 120, 100 * A) for n in (5, 70) for k in ("", "MP_SAOPD_MODEL=lane")]
    for A, knob in ((65, ""), (4, "MP_SAOPD_MODEL=lane"), (4, "")):
        q += [(call(A=A, budget=A * k + extra), knob) for k in (2556, 2557, 2558, 2706, 2707) for extra in (0, A - 1)]
    # the depth limit
    for A in (1, 4, 65):
        q += [(call(A=A, budget=A * k), "") for k in (0x00ffffff - 3, 0x00ffffff - 2, 0x00ffffff - 1, 0x00ffffff)]
    # each knob alone, then the interactions
    sets = ["{}={}".format(k, v) for k, v in ALONE] + INTERACTIONS
    for knobs in sets:
        for S in (100, 118):
            q += [(call(n=n, S=S, have_cost=1), knobs) for n in (5, 300, 9000)]
            q += [(call(S=S, budget=8), knobs), (call(S=S, device_arrays=1), knobs), (call(S=S, A=65, budget=195), knobs),
                  (call(S=S, n_nodes=121, cap=181, qcap=4096, have_cost=1), knobs), (call(S=S, n_nodes=9, cap=13, qcap=256, have_cost=1), knobs)]
    # a seeded sample of everything at once
    rng = np.random.default_rng(20261020)
    for _ in range(3000):
        A = int(rng.choice([1, 2, 4, 5, 64, 65, 80]))
        S = int(rng.choice([int(rng.integers(1, 140)), int(rng.integers(1, 5000))]))
        n = int(np.exp(rng.uniform(0, np.log(20000))))
        budget = int(rng.choice([int(rng.integers(0, 200)), int(np.exp(rng.uniform(0, np.log(300000))))]))
        kept = int(rng.choice([0, 0, int(rng.integers(1, 3000))]))
        cap = 0 if kept == 0 else kept + int(rng.integers(0, 2000))
        qcap = 0 if kept == 0 else int(2 ** rng.integers(8, 18))
        picks = dict(ALONE[i] for i in sorted(rng.choice(len(ALONE), size=int(rng.integers(0, 4)), replace=False)))
        knobs = " ".join("{}={}".format(k, v) for k, v in picks.items())
        q.append((call(n=n, S=S, A=A, budget=budget, n_nodes=kept, cap=cap, qcap=qcap, have_cost=int(rng.integers(0, 2)),
                       device_arrays=int(rng.integers(0, 4) == 0), cus=int(rng.choice([256, 256, 80, 304]))), knobs))
    return q


def set_knobs(knobs):
    for k in KNOBS:
        os.environ.pop(k, None)
    for kv in knobs.split():
        k, v = kv.split("=", 1)
        os.environ[k] = v


def choose(c, knobs):
    """-> (status, error phrase, form, fallback, out) of one query"""
    set_knobs(knobs)
    try:
        form, fallback, out = native.saopd_choose_form(c)
        return 0, "", form, fallback, out
    except native.NativeError as e:
        phrase = [p for p in ERRORS if p in str(e)]
        assert len(phrase) == 1, str(e)
        return e.code, phrase[0], "", "", np.zeros(len(native.SAOPD_FORM_FIELDS), dtype=np.int64)
    finally:
        set_knobs("")


def main():
    q = queries()
    rows = [choose(c, k) for c, k in q]
    out = dict(call=np.array([c for c, _ in q], dtype=np.int64), knobs=np.array([k for _, k in q]),
               status=np.array([r[0] for r in rows], dtype=np.int32), error=np.array([r[1] for r in rows]),
               form=np.array([r[2] for r in rows]), fallback=np.array([r[3] for r in rows]),
               out=np.array([r[4] for r in rows], dtype=np.int64))
    path = os.path.join(REPO, "tests", "golden", "saopd_forms.npz")
    np.savez_compressed(path, **out)
    forms, counts = np.unique(out["form"], return_counts=True)
    errors, ecounts = np.unique(out["error"], return_counts=True)
    print(path, len(q), "queries", dict(zip(forms.tolist(), counts.tolist())), dict(zip(errors.tolist(), ecounts.tolist())))


if __name__ == "__main__":
    main()
