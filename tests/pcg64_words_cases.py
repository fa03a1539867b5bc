"""The PCG64 step on four 32-bit words (csrc/pcg64.hpp, Pcg64W) restated on Python integers, and the generator states that
exercise every carry of it.  Written once and used by tests/test_pcg64_words.py (against Python integers and numpy), by
tests/test_pcg64_words_host.py (the header itself on the host, against unsigned __int128) and by tests/test_gpu_uct_pcg_words.py
(the rollouts of uct_kernel, against the oracle).

The step: ten multiply-adds by columns of 32-bit limbs, as in Pcg64::mul_add, with
  c1  the 65th bit of column 1 (weight 2^96: bit 0 of word 3),
  k0, k1, k2  the carries of the 32-bit chain that adds the increment to words 0, 1, 2,
  wrap3  whether r3 + inc3 + k2 passes 2^32 (dropped: the state is taken modulo 2^128)."""
import random

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MULT = 0x2360ED051FC65DA44385DF649FCCF645
M = [(MULT >> (32 * i)) & M32 for i in range(4)]
FLAGS = ("c1", "k0", "k1", "k2")
# Column 1 is w0 m1 + hi(w0 m0) + w1 m0 <= (2^32 - 1)(m0 + m1) + 2^32 - 1, and for PCG64's multiplier m0 + m1 = 0xE352D5A9 < 2^32:
# the sum stays below 2^64 and c1 is 0 for EVERY state.  The step keeps the compare (it is exact for any multiplier, as the jump
# multipliers of Pcg64::mul_add need it); no record can set it, and the case list holds none.
C1_NEVER = M[0] + M[1] < (1 << 32)


def words(x):
    return [(x >> (32 * i)) & M32 for i in range(4)]


def words_step(state, inc):
    """-> (new state, dict of c1, k0, k1, k2, wrap3, r3): Pcg64W::advance line by line"""
    w, i = words(state), words(inc)
    a0 = w[0] * M[0]
    b = w[0] * M[1] + (a0 >> 32)
    assert b <= M64                                  # "no overflow"
    a1_full = w[1] * M[0] + b
    c1, a1 = a1_full >> 64, a1_full & M64
    c = (w[0] * M[2] + (a1 >> 32)) & M64
    d = (w[1] * M[1] + c) & M64
    a2 = (w[2] * M[0] + d) & M64
    q = (w[0] * M[3] + w[1] * M[2] + w[2] * M[1] + w[3] * M[0]) & M64
    r3 = ((q & M32) + (a2 >> 32) + c1) & M32
    t0 = (a0 & M32) + i[0]
    t1 = (a1 & M32) + i[1] + (t0 >> 32)
    t2 = (a2 & M32) + i[2] + (t1 >> 32)
    t3 = r3 + i[3] + (t2 >> 32)
    new = (t0 & M32) | ((t1 & M32) << 32) | ((t2 & M32) << 64) | ((t3 & M32) << 96)
    return new, dict(c1=c1, k0=t0 >> 32, k1=t1 >> 32, k2=t2 >> 32, wrap3=t3 >> 32, r3=r3)


def words_output(state):
    """-> (lo, hi) of the 64-bit output of `state`: Pcg64W::output line by line"""
    w = words(state)
    xl, xh = w[0] ^ w[2], w[1] ^ w[3]
    rot = w[3] >> 26
    a, b = (xh, xl) if w[3] >> 31 else (xl, xh)

    def alignbit(hi, lo, s):
        return (((hi << 32) | lo) >> (s & 31)) & M32
    return alignbit(b, a, rot), alignbit(a, b, rot)


def step(state, inc):
    return (state * MULT + inc) & M128


def output(state):
    hi, lo = state >> 64, state & M64
    x, r = hi ^ lo, hi >> 58
    return ((x >> r) | (x << ((64 - r) & 63))) & M64


def with_inc3(inc, i3):
    return (inc & ((1 << 96) - 1)) | ((i3 & M32) << 96)


def _search():
    g = random.Random(0x5eed0fca5e5)

    def draw():
        return g.getrandbits(128), g.getrandbits(128) | 1
    cases = [("ones", M128, M128), ("zero_state", 0, 1), ("ones_state_inc1", M128, 1), ("zero_state_ones_inc", 0, M128)]
    for flag in FLAGS:
        for want in (0, 1):
            if (flag, want) == ("c1", 1):            # cannot happen with this multiplier: see C1_NEVER
                continue
            while True:
                s, i = draw()
                if words_step(s, i)[1][flag] == want:
                    cases.append(("{}={}".format(flag, want), s, i))
                    break
    for want in (0, 1):                              # every carry at once
        while True:
            s, i = draw()
            f = words_step(s, i)[1]
            if all(f[k] == want for k in FLAGS[1:]):
                cases.append(("all={}".format(want), s, i))
                break
    # the last word: r3 + inc3 + k2.  inc3 touches nothing else, so it is chosen after r3 and k2 are known.
    for k2 in (0, 1):
        while True:
            s, i = draw()
            f = words_step(s, i)[1]
            if f["k2"] == k2:
                break
        # the sum lands exactly on 2^32 (word 3 = 0) -- through the carry alone where k2 = 1 -- one below it, and far beyond it
        cases.append(("w3_exact_k2={}".format(k2), s, with_inc3(i, (1 << 32) - f["r3"] - k2)))
        cases.append(("w3_below_k2={}".format(k2), s, with_inc3(i, M32 - f["r3"] - k2)))
        cases.append(("w3_far_k2={}".format(k2), s, with_inc3(i, M32)))
    # rotations of the output: the top six bits of the NEW word 3
    for rot in (0, 31, 32, 63):
        for low in (0, (1 << 26) - 1):
            s, i = draw()
            f = words_step(s, i)[1]
            cases.append(("rot{}_{}".format(rot, "lo" if low == 0 else "hi"), s, with_inc3(i, ((rot << 26) | low) - f["r3"] - f["k2"])))
    cases += [("random{}".format(j),) + draw() for j in range(24)]
    return cases


CASES = _search()          # (name, state, increment): 128-bit integers, increment odd


def record_of(state, inc, back=0):
    """The project's six-word record (state hi, lo, inc hi, lo, has_uint32, uinteger) from which the (back + 1)-th step is the
    step of `state` (back = 0: the record's own first step)."""
    inv = pow(MULT, -1, 1 << 128)
    for _ in range(back):
        state = ((state - inc) * inv) & M128
    return [state >> 64, state & M64, inc >> 64, inc & M64, 0, 0]
