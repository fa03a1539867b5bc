"""Forged numpy ``Generator(PCG64)`` records: generator states whose NEXT outputs are chosen, so that a test reaches the draws no
seed ever meets -- a rejection of the bounded draw (probability (2^32 mod k) / 2^32 per word), a rejection that crosses the halves
of one 64-bit output or starts at the buffered half, and ``random()`` exactly on a cdf threshold (probability 2^-53).

PCG64 steps ``state <- state * MULT + inc (mod 2^128)`` and outputs ``rotr64(hi ^ lo, hi >> 58)`` of the NEW state.  MULT is odd, so
the step has an inverse; and for any wanted output ``o`` and any ``hi``, ``lo = hi ^ rotl64(o, hi >> 58)`` is a state whose output
is ``o``.  Stepping that state back gives the record to hand to a planner.  Python integers only; tests/test_forge_host.py checks
every function here against numpy itself.

A generator that a planner seeds ON THE DEVICE from a draw of the record (a model clone) is reached the other way round: the
record fixes the seed, ``clone_k53`` asks numpy for the clone's draw, and ``row_on`` builds the model row that this draw meets
exactly on a cdf entry (tests/forged_clone_cases.py).

A record is the project's six words: state hi, state lo, inc hi, inc lo, has_uint32, uinteger."""

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MULT = 0x2360ED051FC65DA44385DF649FCCF645
MULT_INV = pow(MULT, -1, 1 << 128)
DEFAULT_HI = 0x9E3779B97F4A7C15        # any value serves; its top six bits (39) are the rotation of the forged output
DEFAULT_INC = (0x5851F42D4C957F2D << 64) | 0x14057B7EF767814F     # numpy's increment is odd; any odd value serves


def rotl64(x, r):
    r &= 63
    return ((x << r) | (x >> ((64 - r) & 63))) & M64


def rotr64(x, r):
    return rotl64(x, (64 - r) & 63)


def step(state, inc):
    return (state * MULT + inc) & M128


def step_back(state, inc):
    return ((state - inc) * MULT_INV) & M128


def output(state):
    hi, lo = state >> 64, state & M64
    return rotr64(hi ^ lo, hi >> 58)


def record(inc, out64, hi=DEFAULT_HI, buffered=None, skip=0):
    """The record whose (skip + 1)-th 64-bit output from now is ``out64`` (``skip`` ordinary outputs come first).  ``buffered=x``:
    the record enters with has_uint32 = 1, uinteger = x, so the next 32-bit draw is x and comes before any output."""
    inc |= 1
    assert 0 <= out64 <= M64 and 0 <= hi <= M64 and 0 < inc <= M128
    state = (hi << 64) | (hi ^ rotl64(out64, hi >> 58))
    assert output(state) == out64
    for _ in range(skip + 1):
        state = step_back(state, inc)
    has, word = (0, 0) if buffered is None else (1, int(buffered))
    assert 0 <= word < (1 << 32)
    return [state >> 64, state & M64, inc >> 64, inc & M64, has, word]


def words_record(inc, low, high, hi=DEFAULT_HI, buffered=None, skip=0):
    """record() by the two 32-bit draws the forged output serves: ``low`` first, then ``high`` (numpy's buffered half)."""
    return record(inc, (high << 32) | low, hi=hi, buffered=buffered, skip=skip)


def double_record(inc, k53, low11, hi=DEFAULT_HI, buffered=None, skip=0):
    """A record for which the (skip + 1)-th ``random()`` is exactly ``k53 * 2^-53``; ``low11``: the 11 bits random() drops."""
    assert 0 <= k53 < (1 << 53) and 0 <= low11 < (1 << 11)
    return record(inc, (k53 << 11) | low11, hi=hi, buffered=buffered, skip=skip)


def lemire_threshold(k):
    return (1 << 32) % k


def leftover(x, k):
    return (x * k) & 0xffffffff


def _edge_words(k):
    """The words x = ceil(j * 2^32 / k): the only ones whose leftover (x * k mod 2^32) is below k."""
    for j in range(k):
        x = -((-j << 32) // k)
        if x < (1 << 32):
            assert leftover(x, k) < k
            yield x


def rejecting_words(k, n):
    """Up to ``n`` 32-bit words that ``integers(0, k)`` REJECTS: (x * k) mod 2^32 < 2^32 mod k.  None for a power of two; x = 0
    for every other k."""
    thr, out = lemire_threshold(k), []
    for x in _edge_words(k):
        if len(out) >= n:
            break
        if leftover(x, k) < thr:
            out.append(x)
    return out


def accepting_edge_words(k):
    """Words whose leftover is below k but not below the threshold, by ascending leftover: they enter the ``if`` of the bounded
    draw and skip its loop.  The first one's leftover EQUALS the threshold wherever such a word exists (it does for every k the
    tests use): a loop written with ``<=`` would reject it.  (Every edge word for a power of two, whose threshold is 0.)"""
    thr = lemire_threshold(k)
    return sorted((x for x in _edge_words(k) if leftover(x, k) >= thr), key=lambda x: leftover(x, k))


def plain_word(k, value):
    """A word that ``integers(0, k)`` accepts without entering the ``if`` and maps to ``value``."""
    x = -((-value << 32) // k) + 1      # one above the edge word of `value`: leftover in [k, 2k)
    assert (x * k) >> 32 == value and leftover(x, k) >= k, (k, value)
    return x


class Stream(object):
    """numpy's Generator over a record, restated on Python integers, counting what it does: ``outputs`` (64-bit outputs drawn) and
    ``rejections`` (words the bounded draw threw away).  The PREDICTION the host tests hold numpy, the oracle and the device
    multiply to; a drop-in ``np_random`` for the planner restatements (integers / choice / random)."""

    def __init__(self, rec, next64=None):
        self.state, self.inc = (int(rec[0]) << 64) | int(rec[1]), (int(rec[2]) << 64) | int(rec[3])
        self.has_uint32, self.uinteger = int(rec[4]), int(rec[5])
        self.outputs = self.rejections = self.entered_if = 0
        self._next64 = next64

    def record(self):
        return [self.state >> 64, self.state & M64, self.inc >> 64, self.inc & M64, self.has_uint32, self.uinteger]

    def next64(self):
        self.outputs += 1
        if self._next64 is not None:        # another restatement of the step (the device's), same bookkeeping
            hi, lo = self._next64(self.state >> 64, self.state & M64, self.inc >> 64, self.inc & M64)
            self.state = (hi << 64) | lo
        else:
            self.state = step(self.state, self.inc)
        return output(self.state)

    def next32(self):
        if self.has_uint32:
            self.has_uint32 = 0
            return self.uinteger
        n = self.next64()
        self.has_uint32, self.uinteger = 1, n >> 32
        return n & 0xffffffff

    def below(self, k):
        if k <= 1:
            return 0
        m = self.next32() * k
        if (m & 0xffffffff) < k:
            self.entered_if += 1
            thr = lemire_threshold(k)
            while (m & 0xffffffff) < thr:
                self.rejections += 1
                m = self.next32() * k
        return m >> 32

    def random(self):
        return (self.next64() >> 11) * (1.0 / 9007199254740992.0)

    # ---- the part of numpy.random.Generator the planner restatements use
    def integers(self, low, high=None):
        assert high is None
        return self.below(int(low))

    def choice(self, a, p=None):
        import numpy as np
        n = int(a) if np.ndim(a) == 0 else len(a)
        if p is None:
            i = self.below(n)
        else:
            cdf = np.asarray(p, dtype=np.float64).cumsum()
            cdf /= cdf[-1]
            i = int(np.searchsorted(cdf, self.random(), side="right"))
        return i if np.ndim(a) == 0 else a[i]


class LoggingStream(Stream):
    """A Stream that logs every draw a planner restatement makes: ``log`` holds (kind, words, outputs, arg, rejections) -- where in
    the stream the draw begins: ``words`` 32-bit draws were made before it (a 64-bit output counts as two; a half the record
    entered with is draw 0) and ``outputs`` 64-bit outputs; ``arg`` is the ``k`` of a bounded draw ("below") or the ``p`` of a
    weighted choice ("choice"); ``rejections``: the words the bounded draw threw away."""

    def __init__(self, rec, next64=None):
        Stream.__init__(self, rec, next64)
        self.log, self._entry = [], self.has_uint32

    def words(self):
        return 2 * self.outputs + self._entry - self.has_uint32

    def below(self, k):
        at, before = (self.words(), self.outputs), self.rejections
        value = Stream.below(self, k)
        if k > 1:
            self.log.append(("below",) + at + (int(k), self.rejections - before))
        return value

    def choice(self, a, p=None):
        if p is None:
            return Stream.choice(self, a)
        import numpy as np
        self.log.append(("choice", self.words(), self.outputs, np.array(p, dtype=np.float64), 0))
        return Stream.choice(self, a, p)


# ---- the generator of a clone that a planner seeds on the device, and model rows forged to its draws ----------------------------
TWO53 = 1 << 53


def clone_k53(x, n=0):
    """The 53-bit integer of the n-th ``random()`` (from 0) of ``Generator(PCG64(SeedSequence(x)))``: what a clone seeded with the
    planner's draw ``x`` draws at its (n + 1)-th model step.  numpy's own, exact: random() is k53 * 2^-53."""
    import numpy as np
    u = float(np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(x)))).random(n + 1)[n])
    k53 = int(u * float(TWO53))
    assert k53 * 2.0 ** -53 == u
    return k53


def row_on(k53, W, b, zeros=()):
    """A float64 row of ``W`` probabilities n_j * 2^-53 with integer n_j >= 0, sum n_j = 2^53 and n_0 + .. + n_b = ``k53``: every
    partial sum is exact, cdf[-1] == 1.0 and cdf[b] == k53 * 2^-53.  ``zeros``: indices that get n_j = 0 (not ``b``; a zero at
    b + 1 makes cdf[b + 1] == cdf[b]).  A draw of k53 * 2^-53 sits ON cdf[b]: searchsorted 'right' passes it (and the zeros
    behind it), 'left' stops at b.  The twin row_on(k53 + 1, ...) has the same draw one step below cdf[b]: both stop at b."""
    import numpy as np
    zeros = set(int(z) for z in zeros)
    assert 0 <= b <= W - 2 and b not in zeros and all(0 <= z < W for z in zeros)
    head = [j for j in range(b + 1) if j not in zeros]
    tail = [j for j in range(b + 1, W) if j not in zeros]
    assert tail and len(head) <= k53 and len(tail) <= TWO53 - k53, (k53, W, b)
    n = [0] * W
    for idx, total in ((head, k53), (tail, TWO53 - k53)):
        for j in idx:
            n[j] = total // len(idx)
        n[idx[-1]] += total - (total // len(idx)) * len(idx)       # (head: the remainder goes to b itself)
    assert sum(n) == TWO53 and sum(n[:b + 1]) == k53 and n[b] >= 1
    row = np.array([float(x) for x in n], dtype=np.float64) * 2.0 ** -53
    assert [int(x * float(TWO53)) for x in row] == n
    return row


def passed(row, b):
    """The index numpy answers for a draw ON cdf[b] of ``row``: b + 1, and past every zero entry that follows."""
    j = b + 1
    while row[j] == 0.0:
        j += 1
    return j


def threshold53(c):
    """ceil(c * 2^53) for a cdf entry c in [0, 1]: random() = k * 2^-53 is below c exactly when k is below it (exact: Fractions)."""
    from fractions import Fraction
    f = Fraction(float(c)) * (1 << 53)
    return -((-f.numerator) // f.denominator)


# ---- the cases every test forges: how many words a bounded draw among k rejects, and where they sit ------------------------
TIE_CASES = ("seeded", "reject0", "reject1", "reject2", "reject3", "accept_edge", "buffered_plain")


def tie_case_record(case, k, inc=DEFAULT_INC, skip=0, salt=0, lead=0):
    """The record of one of TIE_CASES for a draw among ``k`` that follows ``skip`` 64-bit outputs and then ``lead`` 32-bit draws
    (a planner's per-episode seed draw, say); -> (record, rejections expected of that draw, or None for the control).

    A record prescribes three consecutive 32-bit draws at most: the buffered word, then the low and the high half of the forged
    output.  The ``lead`` draws get ordinary words, the draw among k gets, by case: reject<n> = n rejected words, then an accepted
    one (reject3 without ``lead``: buffered word, low half, high half; reject2: low and high half, the accepted word is the next
    output's; with ``lead`` the rejections that no longer fit are dropped); reject0 = an ordinary word; accept_edge = a word
    that enters the ``if`` and skips the loop; buffered_plain = an ordinary word from the buffer (the halves behind it reject,
    for the next draw among k); seeded = numpy's own record of seed ``salt`` (control).  A power of two has no rejecting word:
    x = 0 stands in and no rejection is expected."""
    import numpy as np
    if case == "seeded":
        st = np.random.PCG64(np.random.SeedSequence(salt)).state
        s, i = st["state"]["state"], st["state"]["inc"]
        return [s >> 64, s & M64, i >> 64, i & M64, st["has_uint32"], st["uinteger"]], None
    rej = rejecting_words(k, 3)
    pow2 = not rej
    if pow2:
        rej = [0]
    r = [rej[(i + salt) % len(rej)] for i in range(3)]
    plain = plain_word(k, (1 + salt) % k)
    edge = accepting_edge_words(k)
    words = {"reject0": [plain], "reject1": [r[0], plain], "reject2": [r[0], r[1]], "reject3": [r[0], r[1], r[2]],
             "accept_edge": [edge[salt % len(edge)]], "buffered_plain": [plain, r[0], plain]}[case]
    seq = [0x12345678 + 2 * j + salt for j in range(lead)] + words
    use_buffer = len(seq) >= 3 or case in ("reject3", "buffered_plain")
    slots = (seq + [plain, plain, plain])[:3 if use_buffer else 2]
    landed = slots[lead:lead + len(words)]
    expect = 0
    if not pow2 and case.startswith("reject"):
        n = int(case[-1])
        expect = min(n, len(landed))
    hi = (DEFAULT_HI + salt * 0x0400000000000001) & M64
    if use_buffer:
        return words_record(inc, slots[1], slots[2], hi=hi, buffered=slots[0], skip=skip), expect
    return words_record(inc, slots[0], slots[1], hi=hi, skip=skip), expect


def tie_batch(k, n, skip=0, lead=0):
    """``n`` records cycling through TIE_CASES (different increments and words per root) -> (uint64 [n, 6], case names).
    With ``lead`` draws before the tie a record has no room for three rejections: reject3 would repeat reject2 and is left out."""
    import numpy as np
    cases = [c for c in TIE_CASES if not (lead and c == "reject3")]
    recs, names = [], []
    for i in range(n):
        case = cases[i % len(cases)]
        inc = (DEFAULT_INC + 2 * i * 0x9E3779B97F4A7C15F39CC0605CEDC834) & M128
        recs.append(tie_case_record(case, k, inc=inc, skip=skip, salt=i // len(cases), lead=lead)[0])
        names.append(case)
    return np.array(recs, dtype=np.uint64), names
