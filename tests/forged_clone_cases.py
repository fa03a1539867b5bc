"""The cases of tests/test_gpu_forged_clone_draws.py, built on the host: models forged to the draws of a clone that a planner seeds
on the device, and records that put a later draw of a plan where a test wants it.  tests/test_forge_host.py checks every case
against numpy and pins the draw each restatement meets it with; the GPU tests hand the same cases to the kernels.

A planner seeds its model clone with ``x = next32() >> 2`` of its own generator (``integers(2 ** 30)``), so a forged record fixes
``x``, numpy gives the clone's n-th ``random()`` as ``forge.clone_k53(x, n)``, and ``forge.row_on`` builds the model row that this
very draw meets ON a cdf entry (the twin row: one step below it).  No seed reaches either: 2^-53 per draw."""
import numpy as np

from tests import forge

SEED_WORDS = (0, 4, 0xFFFFFFFF, 0x9E3779B9)          # x = word >> 2: 0, 1, 2^30 - 1 and an ordinary seed
DENSE_W = 150
DENSE_BS = (0, 62, 63, 64, 127, 148)                 # the count crosses a ballot of 64; 63 / 127: a ballot full to its last lane
SPARSE_BS = {1: (), 3: (0, 1), 4: (0, 1, 2), 5: (0, 1, 2, 3)}
TIE_KS = (3, 6, 7, 70, 150)


def inc_of(i):
    return (forge.DEFAULT_INC + 2 * i * 0x9E3779B97F4A7C15F39CC0605CEDC834) & forge.M128


def hi_of(i):
    return (forge.DEFAULT_HI + i * 0x0400000000000001) & forge.M64


def zeros_for(W, b, odd):
    """Every other case: a zero entry inside the prefix and one directly behind b (equal adjacent thresholds), where they fit."""
    if not odd:
        return ()
    z = [b // 2] if b >= 2 else ([0] if b == 1 else [])
    if b + 2 < W:
        z.append(b + 1)
    return tuple(z)


def base_model(kind, n_states, n_actions, W, seed):
    """Ordinary rows everywhere: a dense [S, A, S] (W = S) or sparse [S, A, W] model, no terminal state, rewards in [0, 1).
    A sparse row's successors are distinct, so that two outcome indices are two states."""
    g = np.random.Generator(np.random.PCG64(seed))
    reward = g.random((n_states, n_actions))
    if kind == "sparse":
        p = g.random((n_states, n_actions, W)) + 0.05
        p /= p.sum(axis=2, keepdims=True)
        s, a, j = np.ogrid[:n_states, :n_actions, :W]
        nxt = ((s * 7 + a * 3 + j * 11 + 1) % n_states).astype(np.int64)
        assert n_states > 11 * W and all(len(set(row)) == W for row in nxt.reshape(-1, W))
        return dict(mode="sparse", transition=p, next=nxt, reward=reward, terminal=None)
    assert W == n_states
    p = g.gamma(0.3, size=(n_states, n_actions, n_states)) + 1e-6
    p /= p.sum(axis=2, keepdims=True)
    return dict(mode="stochastic", transition=p, next=None, reward=reward, terminal=None)


def one_hot_row(W, j):
    row = np.zeros(W)
    row[j] = 1.0
    return row


# ---- BRUE and stochastic OLOP: the clone's draw at a step of the first rollout / episode -----------------------------------------
def clone_twins(kind, W, n_actions, first="word", step=0, seed=700):
    """Twin roots for every (seed word, b): root i starts in state i, its record's low word is the seed word and its high word
    the ordinary word that draws action ``i % n_actions`` (``first`` = "word": BRUE's integers(|A|), OLOP's uniform
    continuation) or is not drawn at all ("zeros": OLOP's action 0).  Row (i, a_i) is forged to the clone's first draw
    (``step`` 0), or is one-hot onto state n + i whose row for the SECOND action -- an ordinary draw of the record -- is forged
    to the clone's second draw (``step`` 1).  Without a b to forge (a sparse row of one successor) every seed word plans once on
    the ordinary model.
    -> dict(cfg, roots, records, cases=[dict(root, x, b, twin, state, action, row, want)])"""
    bs = DENSE_BS if kind == "stochastic" else SPARSE_BS[W]
    plan = [(w, b, twin) for w in SEED_WORDS for b in bs for twin in (0, 1)] or [(w, None, 0) for w in SEED_WORDS]
    n = len(plan)
    n_states = W if kind == "stochastic" else 67
    assert n * (1 + step) <= min(n_states, 64 * (1 + step)) and n <= 64
    cfg = base_model(kind, n_states, n_actions, W, seed)
    records, cases = [], []
    for i, (word, b, twin) in enumerate(plan):
        a = i % n_actions if first == "word" else 0
        rec = forge.words_record(inc_of(i), word, forge.plain_word(n_actions, i % n_actions), hi=hi_of(i))
        records.append(rec)
        x = word >> 2
        if b is None:
            cases.append(dict(root=i, x=x, b=None, twin=0, state=i, action=a, row=cfg["transition"][i, a].copy(), want=None))
            continue
        state, action = i, a
        if step == 1:
            st = forge.Stream(rec)
            assert st.below(1 << 30) == x and st.below(n_actions) == a
            state, action = n + i, st.below(n_actions)
            if kind == "sparse":
                cfg["transition"][i, a] = one_hot_row(W, 0)
                cfg["next"][i, a, 0] = state
            else:
                cfg["transition"][i, a] = one_hot_row(W, state)
        row = forge.row_on(forge.clone_k53(x, step) + twin, W, b, zeros_for(W, b, (i // 2) % 2 == 1))
        cfg["transition"][state, action] = row
        cases.append(dict(root=i, x=x, b=b, twin=twin, state=state, action=action, row=row,
                          want=b if twin else forge.passed(row, b)))
    return dict(cfg=cfg, roots=np.arange(n, dtype=np.int32), records=np.array(records, dtype=np.uint64), cases=cases)


def one_hot_tie_model(n_states, n_actions, k):
    """tests.helpers.zero_table as a dense model: rows that put probability 1 on the table's successor, rewards all zero, the
    first k actions listed.  -> (cfg, table, available or None)"""
    from tests.helpers import zero_table
    t, r, term, avail = zero_table(n_states, n_actions, k)
    dense = np.zeros((n_states, n_actions, n_states))
    np.put_along_axis(dense, t[:, :, None], 1.0, axis=2)
    return dict(mode="stochastic", transition=dense, next=None, reward=r, terminal=None), (t, r, term), (avail if k < n_actions else None)


# ---- Sparse Sampling: the clone of ONE sample of the root ---------------------------------------------------------------------------
SS_C, SS_A = 65, 2
SS_TARGETS = (0, 1, 63, 64, 65)          # lanes 0, 1, 63 of the first chunk; 64: first lane of the second, action 0's last sample;
SS_TARGETS_H2 = (0, 1, 63, 64)           # 65: action 1's first.  Horizon 2: the top level's C samples of action 0 on C lanes
SS_WORDS = (0, 0xFFFFFFFF)               # seeds 0 and 2^30 - 1
SS_WS = (2, 3, 150)


def ss_bs(W):
    return sorted({b for b in (0, W // 2 - 1, W // 2, W - 2) if 0 <= b <= W - 2})


def ss_record(t, buffered, word, i):
    """The record whose t-th 32-bit draw from now (from 0) is ``word``; ``buffered``: it enters holding a half, draw 0."""
    other = [0x5EED0001 + 8 * i, 0x0DDBA115 + 8 * i, 0xB0FFE4ED ^ (i << 4)]
    if buffered and t == 0:
        return forge.words_record(inc_of(i), other[0], other[1], hi=hi_of(i), buffered=word)
    idx = t - 1 if buffered else t
    low, high = (other[0], word) if idx & 1 else (word, other[0])
    return forge.words_record(inc_of(i), low, high, hi=hi_of(i), buffered=other[2] if buffered else None, skip=idx >> 1)


def ss_cases(W, horizon=1):
    """(t, buffered, word, b, twin, zeros) for every target sample, entry, seed word, b and twin of rows of width W."""
    out = []
    for t in (SS_TARGETS if horizon == 1 else SS_TARGETS_H2):
        for buffered in (False, True):
            for word in SS_WORDS:
                for b in ss_bs(W):
                    for twin in (0, 1):
                        out.append((t, buffered, word, b, twin, zeros_for(W, b, len(out) % 4 >= 2)))
    return out


def ss_batches(kind, W, horizon=1, seed=800):
    """The cases of ``ss_cases`` in batches of at most 64 roots, one root state per case (a dense model of W states holds W cases).
    Root i of a batch starts in state i; row (i, action of the target sample) is forged to that sample's clone.
    -> [dict(cfg, roots, records, cases=[dict(root, t, x, b, twin, action, row, want, buffered)])]"""
    todo = ss_cases(W, horizon)
    n_states = W if kind == "stochastic" else 67
    per = min(n_states, 64)
    batches = []
    for lo in range(0, len(todo), per):
        cfg = base_model(kind, n_states, SS_A, W, seed + lo)
        records, cases = [], []
        for i, (t, buffered, word, b, twin, zeros) in enumerate(todo[lo:lo + per]):
            action = t // SS_C
            row = forge.row_on(forge.clone_k53(word >> 2) + twin, W, b, zeros)
            cfg["transition"][i, action] = row
            records.append(ss_record(t, buffered, word, lo + i))
            cases.append(dict(root=i, t=t, x=word >> 2, b=b, twin=twin, action=action, row=row, buffered=buffered,
                              want=b if twin else forge.passed(row, b)))
        batches.append(dict(cfg=cfg, roots=np.arange(len(cases), dtype=np.int32), records=np.array(records, dtype=np.uint64),
                            cases=cases))
    return batches


# ---- Sparse Sampling: the root's tie, after samples that consume a known number of words -----------------------------------------
SS_TIE_C = 3
SS_TIE_CASES = tuple(c for c in forge.TIE_CASES if c != "reject3")     # three rejections need the buffered word: the samples took it


def ss_tie_record(case, k, n_words, i, salt):
    """forge.tie_case_record for a tie among k that follows ``n_words`` 32-bit draws -> (record, rejections expected or None).
    An odd count is tie_case_record's ``lead``: the tie starts at the forged output's high half (a record that enters with a
    buffered word gives that word to sample 0).  After an even count the tie starts at the forged output's low half; there
    "buffered_plain" -- the tie's word comes from the buffered half -- is a record that enters with a half of its own, so that the
    samples end on a low half and the tie takes the ordinary word forged into the high one."""
    if case == "buffered_plain" and n_words % 2 == 0:
        plain = forge.plain_word(k, (1 + salt) % k)
        return forge.words_record(inc_of(i), 0x12345678 + salt, plain, hi=hi_of(salt), buffered=0x0BADF00D + i,
                                  skip=n_words // 2 - 1), 0
    return forge.tie_case_record(case, k, inc=inc_of(i), skip=n_words // 2, salt=salt, lead=n_words % 2)


def ss_tie_batch(k, n, n_words):
    recs, names, expect = [], [], []
    for i in range(n):
        case = SS_TIE_CASES[i % len(SS_TIE_CASES)]
        rec, e = ss_tie_record(case, k, n_words, i, i // len(SS_TIE_CASES))
        recs.append(rec); names.append(case); expect.append(e)
    return np.array(recs, dtype=np.uint64), names, expect


# ---- BRUE's estimate() choice on an exact boundary, through the planner ---------------------------------------------------------
EST = dict(horizon=3, budget=6, gamma=0.9, skip=5)


def estimate_chain():
    """0 -> 1; 1 -> {2, 3} at 0.5 each; 2 -> 4; 3 -> 5; 4 and 5 absorb.  R(2) = 0.25, R(3) = 0.75, one action."""
    S = 6
    p = np.zeros((S, 1, S))
    for s, t in ((0, 1), (2, 4), (3, 5), (4, 4), (5, 5)):
        p[s, 0, t] = 1.0
    p[1, 0, 2] = p[1, 0, 3] = 0.5
    r = np.zeros((S, 1))
    r[2, 0], r[3, 0] = 0.25, 0.75
    return dict(mode="stochastic", transition=p, next=None, reward=r, terminal=None)


def estimate_sides(rec):
    """The states the two rollouts of the record reach from state 1: each rollout draws one seed word and three doubles of the
    planner's generator whatever their values (one action: integers(1) draws nothing; estimate() runs 2 + 1 + 0 choices)."""
    st, sides = forge.Stream(rec), []
    for _ in range(2):
        x = st.below(1 << 30)
        sides.append(2 if forge.clone_k53(x, 1) < (1 << 52) else 3)
        for _ in range(3):
            st.random()
    return sides


def estimate_records(n_pairs=4, search=4096):
    """Records whose 6th 64-bit output -- the second rollout's choice over state 1's two outcomes -- is 2^52 (u == cdf[0]: numpy
    picks index 1) and 2^52 - 1 (index 0), and whose two rollouts leave state 1 on different sides: outcome counts (1, 1).  The
    forged state's high word is searched for that.  -> (records [2 * n_pairs, 6], k53 of each)"""
    recs, ks = [], []
    for pair in range(n_pairs):
        for j in range(search):
            hi = (hi_of(pair) + (j + 1) * 0x2545F4914F6CDD1D) & forge.M64
            pairs = [forge.double_record(inc_of(pair), k53, 0x7ff * (pair & 1), hi=hi, skip=EST["skip"]) for k53 in ((1 << 52), (1 << 52) - 1)]
            if all(sorted(estimate_sides(r)) == [2, 3] for r in pairs):
                break
        else:
            raise AssertionError("no state found whose two rollouts part at state 1")
        recs += pairs
        ks += [1 << 52, (1 << 52) - 1]
    return np.array(recs, dtype=np.uint64), ks
