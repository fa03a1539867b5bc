#!/usr/bin/env python3
"""The kernel form mp_uct_plan chooses, pinned for tests/test_uct_forms.py (host only: no GPU is needed or used).

    python3 tests/golden/gen/make_golden_uct_forms.py

-> tests/golden/uct_forms.npz, one row per query:
   call   int32 [N, 14]  the call's description (native.UCT_CALL_FIELDS)
   knobs  str   [N]      the MP_UCT_* knobs set for it, "NAME=value" joined by spaces ("" = none)
   status int32 [N]      0, or the error code the plan returns for that shape
   form   str   [N]      the form's name ("" on error)
   out    int32 [N, 7]   native.UCT_FORM_FIELDS (zeros on error)
The queries: every edge of the batch-size, horizon and episode thresholds over the model kinds and |A| values, policies, kept
trees in each layout, each knob alone, the knobs' interactions, and a seeded sample.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, REPO)

from rl_agents_amd import native  # noqa: E402

KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_LONE_WAVES", "MP_UCT_EACH", "MP_UCT_ROW", "MP_UCT_ROWS",
         "MP_UCT_ROW_WAVES", "MP_UCT_ROW_ROOTS", "MP_UCT_PATH", "MP_UCT_LANES", "MP_UCT_LDSR_WAVES", "MP_UCT_CART_REP",
         "MP_UCT_CART_WAVES")

# S, NB, Sb, compact transitions, reward index, distinct rewards, CartPole
MODELS = {
    "headline": (10000, 1, 10000, 1, 1, 7),            # highway-shaped table, at most 256 rewards
    "rewards256": (10000, 1, 10000, 1, 1, 256),
    "many_rewards": (10000, 1, 10000, 1, 0, 0),        # > 256 distinct rewards: no reward index
    "large_S": (40000, 1, 40000, 0, 0, 0),             # S >= 32 768: no compact transitions
    "S1000": (1000, 1, 1000, 1, 1, 12),
    "S250": (250, 1, 250, 1, 1, 3),
    "batch120": (7680, 64, 120, 1, 1, 5),              # 64 MDPs of 120 states
    "batch120_wide": (491520, 4096, 120, 0, 0, 0),
    "batch_large": (80000, 2, 40000, 0, 0, 0),         # Sb >= 32 768
}
ACTIONS = (2, 3, 5, 8, 11, 40)
SUBSET = ("headline", "many_rewards", "S250", "batch120", "cartpole")


def shapes(names=None, actions=ACTIONS):
    """(model facts, |A|) pairs: every table model with every |A|, CartPole with its two actions"""
    for name in (names or list(MODELS) + ["cartpole"]):
        if name == "cartpole":
            yield (0, 1, 0, 0, 0, 0, 1), 2
            continue
        for A in actions:
            yield MODELS[name] + (0,), A


def call(model, A, n, E=33, H=30, pol=0, kept=-1, cus=256):
    S, NB, Sb, t16, r8, nr, cart = model
    return (n, E, H, A, S, NB, Sb, t16, r8, nr, cart, pol, kept, cus)


def roots_edges(cus):
    r = {1, 15, 16, 17, 255, 256, 257, 2048, 2049, 4096, 4097, 16384, 16385, 65535, 65536, 262144}
    for m in (1, 2, 4, 8, 16, 32, 64, 256):
        r |= {cus * m, cus * m + 1}
    r |= {256 * cus - 64, 256 * cus - 63}     # (n + 63) / 64 >= 4 CUs: the LDS-resident default
    return sorted(r)


def spill_horizon(A, E):
    """the first horizon whose [H + 1][64] path stack and tables pass 64 KiB of LDS"""
    te = min(E, 16384 // (8 * (A + 1)))
    H = 1
    while ((H + 1) + 2 * A + (te + 1) + A * (te + 2)) * 8 + (H + 1) * 64 * 4 <= 65536:
        H += 1
    return H


ALONE = [("MP_UCT_MODEL", v) for v in ("global", "ldsr", "other")] + \
        [("MP_UCT_QUAD", v) for v in ("0", "1")] + [("MP_UCT_LONE", v) for v in ("0", "1")] + \
        [("MP_UCT_LONE_WAVES", v) for v in ("0", "1", "2", "3", "4", "8")] + \
        [("MP_UCT_EACH", v) for v in ("0", "1")] + [("MP_UCT_ROW", v) for v in ("0", "1")] + \
        [("MP_UCT_ROWS", v) for v in ("0", "1")] + [("MP_UCT_ROW_WAVES", v) for v in ("1", "2", "3", "4", "8")] + \
        [("MP_UCT_ROW_ROOTS", v) for v in ("2", "3", "4")] + [("MP_UCT_PATH", v) for v in ("spill", "x")] + \
        [("MP_UCT_LANES", v) for v in ("1", "3", "4", "16", "64")] + \
        [("MP_UCT_LDSR_WAVES", v) for v in ("1", "4", "16", "32")] + \
        [("MP_UCT_CART_REP", v) for v in ("0", "2", "4", "6")] + [("MP_UCT_CART_WAVES", v) for v in ("1", "2", "3", "4")]

INTERACTIONS = [
    "MP_UCT_MODEL=global MP_UCT_QUAD=1", "MP_UCT_MODEL=ldsr MP_UCT_QUAD=1", "MP_UCT_MODEL=ldsr MP_UCT_LONE=1",
    "MP_UCT_MODEL=other MP_UCT_ROWS=1", "MP_UCT_MODEL=global MP_UCT_LONE_WAVES=2", "MP_UCT_MODEL=global MP_UCT_EACH=1",
    "MP_UCT_QUAD=1 MP_UCT_LONE=1", "MP_UCT_QUAD=0 MP_UCT_LONE_WAVES=2", "MP_UCT_QUAD=1 MP_UCT_ROWS=1",
    "MP_UCT_ROWS=1 MP_UCT_LONE_WAVES=4", "MP_UCT_ROWS=0 MP_UCT_LONE=1", "MP_UCT_PATH=spill MP_UCT_LONE_WAVES=2",
    "MP_UCT_PATH=spill MP_UCT_ROWS=1", "MP_UCT_PATH=spill MP_UCT_MODEL=global", "MP_UCT_LONE=0 MP_UCT_LONE_WAVES=2",
    "MP_UCT_LONE=1 MP_UCT_LONE_WAVES=2", "MP_UCT_EACH=0 MP_UCT_ROW=1", "MP_UCT_EACH=1 MP_UCT_ROW=0",
    "MP_UCT_ROW_WAVES=8 MP_UCT_ROWS=1", "MP_UCT_ROW_WAVES=8 MP_UCT_ROW=1", "MP_UCT_ROW_WAVES=2 MP_UCT_ROW_ROOTS=4 MP_UCT_ROWS=1",
    "MP_UCT_LANES=16 MP_UCT_CART_REP=2", "MP_UCT_LANES=4 MP_UCT_CART_WAVES=2", "MP_UCT_LANES=16 MP_UCT_MODEL=global",
    "MP_UCT_LDSR_WAVES=8 MP_UCT_MODEL=ldsr", "MP_UCT_LDSR_WAVES=2 MP_UCT_QUAD=1",
]


def queries():
    """-> [(call, knobs)]"""
    q = []
    # defaults at every batch-size edge, on 256 CUs and on fewer
    for cus in (256, 80):
        for model, A in shapes():
            q += [(call(model, A, n, cus=cus), "") for n in roots_edges(cus)]
    for model, A in shapes():
        q += [(call(model, A, n, cus=0), "") for n in (1, 257, 4097, 65536)]
    # horizons and episode counts at their edges
    for model, A in shapes():
        hs = spill_horizon(A, 33)
        for n in (1, 16, 256, 4096, 65536, 262144):
            q += [(call(model, A, n, H=H), "") for H in (1, 63, 64, 255, 256, hs - 1, hs, 7000)]
            q += [(call(model, A, n, E=E, H=H), "") for E in (1, 200, 1000, 5000) for H in (30, spill_horizon(A, E))]
    # policies, plain and listed
    for model, A in shapes([m for m in MODELS]):
        q += [(call(model, A, n, H=H, pol=pol), "") for pol in (1, 2) for n in (1, 256, 4096, 65536) for H in (30, 300)]
    # kept trees in each layout: group-interleaved where |A| has a specialisation, root-major (also a kept CartPole tree, |A| = 2)
    for model, A in shapes():
        for kept in (0, 2) if 2 <= A <= 8 else (0,):
            q += [(call(model, A, n, H=H, kept=kept), "") for n in (1, 256, 4096, 65536, 262144) for H in (30, 300)]
    # each knob alone, then the interactions
    sets = ["{}={}".format(k, v) for k, v in ALONE] + INTERACTIONS
    for knobs in sets:
        for model, A in shapes(SUBSET, (2, 5, 11)):
            q += [(call(model, A, n), knobs) for n in (1, 16, 300, 4096, 65536)]
            q += [(call(model, A, n, H=300), knobs) for n in (16, 4096)]
            q += [(call(model, A, 4096, kept=2 if 2 <= A <= 8 else 0), knobs)]
    # a seeded sample of everything at once
    rng = np.random.default_rng(20261016)
    names = list(MODELS) + ["cartpole"]
    for _ in range(3000):
        model, A = next(shapes([names[rng.integers(len(names))]], (ACTIONS[rng.integers(len(ACTIONS))],)))
        n = int(np.exp(rng.uniform(0, np.log(300000))))
        H = int(rng.choice([int(rng.integers(1, 80)), int(rng.integers(1, 400))]))
        E = int(np.exp(rng.uniform(0, np.log(2000))))
        pol = 0 if model[6] else int(rng.choice([0, 0, 0, 1, 2]))
        kept = int(rng.choice([-1, -1, -1, 0, 2])) if 2 <= A <= 8 else int(rng.choice([-1, 0]))
        cus = int(rng.choice([256, 256, 80, 304]))
        picks = dict(ALONE[i] for i in sorted(rng.choice(len(ALONE), size=int(rng.integers(0, 4)), replace=False)))
        knobs = " ".join("{}={}".format(k, v) for k, v in picks.items())
        q.append((call(model, A, n, E=E, H=H, pol=pol, kept=kept, cus=cus), knobs))
    return q


def set_knobs(knobs):
    for k in KNOBS:
        os.environ.pop(k, None)
    for kv in knobs.split():
        k, v = kv.split("=", 1)
        os.environ[k] = v


def choose(c, knobs):
    """-> (status, form, out) of one query"""
    set_knobs(knobs)
    try:
        form, out = native.uct_choose_form(c)
        return 0, form, out
    except native.NativeError as e:
        return e.code, "", np.zeros(len(native.UCT_FORM_FIELDS), dtype=np.int64)
    finally:
        set_knobs("")


def main():
    q = queries()
    rows = [choose(c, k) for c, k in q]
    out = dict(call=np.array([c for c, _ in q], dtype=np.int32), knobs=np.array([k for _, k in q]),
               status=np.array([r[0] for r in rows], dtype=np.int32), form=np.array([r[1] for r in rows]),
               out=np.array([r[2] for r in rows], dtype=np.int32))
    path = os.path.join(REPO, "tests", "golden", "uct_forms.npz")
    np.savez_compressed(path, **out)
    forms, counts = np.unique(out["form"], return_counts=True)
    print(path, len(q), "queries", dict(zip(forms.tolist(), counts.tolist())))


if __name__ == "__main__":
    main()
