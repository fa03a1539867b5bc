"""Forged generator records (tests/forge.py) on the host: numpy is the reference.

Every record forges a draw that no seeded test meets -- 0 to 3 consecutive rejections of the bounded draw behind a tie break
(buffered word, low half, high half of one output), a word that enters the draw's ``if`` and skips its loop, ``random()`` exactly
on and just below a cdf threshold -- and is then pinned to: numpy's ``Generator`` itself (value, outputs consumed, has_uint32),
the C oracle's ``pcg64_replay`` / ``pchoice_replay``, the host restatements of the device's generator step (the scalar form of
tests/test_host_logic.py and the 32-bit column form restated below, jump-ahead constants included), and the planner
restatements tests/{olop,brue,gbopd}_restatement.py through the generators they take.  tests/test_gpu_forged_draws.py hands
the same records to the kernels.

The last section does the same for the cases of tests/forged_clone_cases.py -- model rows forged to the draws of a clone that a
planner seeds on the device, and later draws of a plan reached with ``skip`` -- which tests/test_gpu_forged_clone_draws.py
hands to BRUE, stochastic OLOP and Sparse Sampling: every twin pair tells searchsorted 'right' from 'left' on numpy itself, and
every restatement is pinned on the draw it meets the forged value with."""
import numpy as np
import pytest

from oracle import oracle
from rl_agents_amd import native
from tests import brue_restatement as brr
from tests import forge
from tests import gbopd_restatement as gbr
from tests import forged_clone_cases as fc
from tests import olop_restatement as olr
from tests import olop_stoch_restatement as osr
from tests import sparse_sampling_restatement as ssr
from tests.helpers import CDF_ROWS as ROWS
from tests.helpers import generator_from, scalar_output, scalar_step, stochastic_model, zero_table

KS = (2, 3, 4, 5, 6, 7, 64, 65, 70, 150)
CASES = [c for c in forge.TIE_CASES if c != "seeded"]
M64 = forge.M64


def outputs_consumed(rec, gen, most=8):
    """How many 64-bit outputs ``gen`` has drawn since ``rec``: the n for which bit_generator.advance(n) of the record gives the
    same 128-bit state."""
    want = gen.bit_generator.state["state"]["state"]
    for n in range(most + 1):
        bg = generator_from(rec).bit_generator
        bg.advance(n)
        if bg.state["state"]["state"] == want:
            return n
    raise AssertionError("more than {} outputs consumed".format(most))


def after(gen):
    return [int(x) for x in native.rng_state_from_generator(gen)]


# ---- the forge itself ------------------------------------------------------------------------------------------------------------
def test_record_forges_the_next_output_of_numpy():
    g = np.random.Generator(np.random.PCG64(5))
    for i in range(200):
        out64 = int(g.integers(0, 1 << 64, dtype=np.uint64))
        hi = int(g.integers(0, 1 << 64, dtype=np.uint64))           # every rotation 0 .. 63 comes up
        inc = (int(g.integers(0, 1 << 64, dtype=np.uint64)) << 64) | int(g.integers(0, 1 << 64, dtype=np.uint64))
        skip = i % 4
        rec = forge.record(inc, out64, hi=hi, skip=skip)
        raw = generator_from(rec).bit_generator.random_raw(skip + 1)
        assert int(raw[-1]) == out64, i
    for out64 in (0, 1, M64, 1 << 63, (1 << 32) - 1, 1 << 32):
        for hi in (0, M64, 31 << 58, 32 << 58, 63 << 58):
            assert int(generator_from(forge.record(forge.DEFAULT_INC, out64, hi=hi)).bit_generator.random_raw()) == out64


def test_word_lists_are_what_they_say():
    for k in KS:
        thr = (1 << 32) % k
        rej = forge.rejecting_words(k, 5)
        assert all((x * k) % (1 << 32) < thr for x in rej)
        assert (rej == []) == (k & (k - 1) == 0)
        if rej:
            assert rej[0] == 0
        edge = forge.accepting_edge_words(k)
        assert edge and all(thr <= (x * k) % (1 << 32) < k for x in edge)
        assert (edge[0] * k) % (1 << 32) == thr        # the word a loop written with <= would reject
        # the enumeration is complete: exactly 2^32 mod k words reject, and k words in all have a leftover below k
        assert len(forge.rejecting_words(k, k + 1)) == thr and len(forge.rejecting_words(k, k + 1)) + len(edge) == k
        for v in range(min(k, 9)):
            x = forge.plain_word(k, v)
            assert (x * k) >> 32 == v and (x * k) % (1 << 32) >= k


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("lead", [0, 1])
def test_bounded_draw_equals_numpy_on_forged_records(k, case, lead):
    """integers(0, k) and choice(k): value, outputs consumed and the buffered half, against the prediction and the oracle."""
    for salt in range(2):
        rec, expect = forge.tie_case_record(case, k, salt=salt, lead=lead)
        pred = forge.Stream(rec)
        for _ in range(lead):
            pred.below(1 << 30)
        assert pred.rejections == 0 and pred.outputs <= 1
        pred.entered_if = 0
        value = pred.below(k)
        assert pred.rejections == expect, (case, k, lead)
        if case == "accept_edge":
            assert pred.entered_if == 1 and pred.rejections == 0
        if case == "reject0":
            assert pred.entered_if == 0
        if k & (k - 1) == 0:
            assert pred.rejections == 0
        if case == "reject3" and lead == 0 and expect == 3:
            assert pred.outputs == 2 and pred.has_uint32 == 1        # buffered word, both halves, then the next output's low half
        if case == "reject2" and lead == 0 and expect == 2:
            assert pred.outputs == 2 and pred.has_uint32 == 1
        if case == "reject1" and lead == 0 and expect == 1:
            assert pred.outputs == 1 and pred.has_uint32 == 0        # low half rejected, high half accepted: the buffer is empty
        for draw in ("integers", "choice"):
            gen = generator_from(rec)
            for _ in range(lead):
                gen.integers(2 ** 30)
            got = int(gen.integers(0, k)) if draw == "integers" else int(gen.choice(k))
            assert got == value, (draw, case, k)
            assert after(gen) == pred.record(), (draw, case, k)
            assert outputs_consumed(rec, gen) == pred.outputs
            assert gen.bit_generator.state["has_uint32"] == pred.has_uint32
        outs, st = oracle.pcg64_replay(rec, [1 << 30] * lead + [k])
        assert int(outs[-1]) == value and [int(x) for x in st] == pred.record(), (case, k)


@pytest.mark.parametrize("k", KS)
def test_second_draw_after_a_buffered_word_rejects_across_a_new_output(k):
    """buffered_plain leaves two rejecting halves behind the first draw: the next draw among k rejects both and accepts from
    the output after them."""
    rec, _ = forge.tie_case_record("buffered_plain", k)
    pred, gen = forge.Stream(rec), generator_from(rec)
    values = [pred.below(k), pred.below(k), pred.below(k)]
    assert [int(gen.integers(0, k)) for _ in range(3)] == values
    assert after(gen) == pred.record()
    outs, st = oracle.pcg64_replay(rec, [k] * 3)
    assert [int(x) for x in outs] == values and [int(x) for x in st] == pred.record()
    if k & (k - 1):
        assert pred.rejections >= 1


def boundary_draws(p):
    """(k53, low11) for every threshold t = ceil(cdf[a] * 2^53) of the row: t and t - 1 where random() can reach them, the 11
    dropped bits all zeros and all ones."""
    draws = []
    for c in oracle.policy_cdf(p):
        t = forge.threshold53(c)
        for k53 in (t - 1, t):
            if 0 <= k53 < (1 << 53):
                draws += [(k53, 0), (k53, 0x7ff)]
    return sorted(set(draws))


@pytest.mark.parametrize("row", sorted(ROWS))
def test_inverse_cdf_boundaries_equal_numpy(row):
    """random() on and just below every threshold: Generator.choice(n, p=row), searchsorted(cdf, u, 'right') and the oracle agree,
    and ``ceil(cdf * 2^53) <= k`` -- the form every kernel restates the search in -- counts the same index."""
    p = ROWS[row]
    cdf = oracle.policy_cdf(p)
    thr = [forge.threshold53(c) for c in cdf]
    draws = boundary_draws(p)
    assert len(draws) >= 2 * len(set(thr)) - 2
    for buffered in (None, 0xdeadbeef):
        for k53, low11 in draws:
            rec = forge.double_record(forge.DEFAULT_INC, k53, low11, buffered=buffered)
            gen = generator_from(rec)
            u = gen.random()
            assert u == k53 * 2.0 ** -53
            assert outputs_consumed(rec, gen) == 1 and after(gen)[4:] == [0 if buffered is None else 1, buffered or 0]
            want = int(np.searchsorted(cdf, u, side="right"))
            assert want == sum(t <= k53 for t in thr), (row, k53)
            if want < len(p):                   # (u at or above cdf[-1] = 1.0 cannot happen: k53 < 2^53)
                assert int(generator_from(rec).choice(len(p), p=p)) == want
            got, st = oracle.pchoice_replay(rec, p, 1)
            assert int(got[0]) == want and [int(x) for x in st] == after(gen), (row, k53, low11)
            pred = forge.Stream(rec)
            assert pred.random() == u and pred.record() == after(gen)
            # what uct.hip's RAWU compares: the raw 64-bit output with thresholds shifted up by 11 bits (a threshold of 2^53
            # does not fit 64 bits shifted: such an entry is never at or below the draw)
            raw = (k53 << 11) | low11
            assert sum((t << 11) <= raw for t in thr if t < (1 << 53)) == want


# ---- the device's generator step, restated ---------------------------------------------------------------------------------------
def column_mul_add(s_hi, s_lo, m, add_lo, add_hi):
    """Pcg64::mul_add of csrc/pcg64.hpp: state * (m3:m2:m1:m0) + add (mod 2^128) by columns of 32-bit limbs, every product one
    32 x 32 + 64 -> 64 multiply-add (wrapping), the carry of column 1 recovered by a compare."""
    def mad(a, b, c):
        return (a * b + c) & M64
    a0, a1, a2, a3 = s_lo & 0xffffffff, s_lo >> 32, s_hi & 0xffffffff, s_hi >> 32
    A0 = mad(a0, m[0], 0)
    B = mad(a0, m[1], A0 >> 32)
    A1 = mad(a1, m[0], B)
    c1 = 1 if A1 < B else 0
    C = mad(a0, m[2], (A1 >> 32) | (c1 << 32))
    D = mad(a1, m[1], C)
    A2 = mad(a2, m[0], D)
    Q = mad(a0, m[3], 0)
    Q = mad(a1, m[2], Q)
    Q = mad(a2, m[1], Q)
    Q = mad(a3, m[0], Q)
    r3 = (Q + (A2 >> 32)) & 0xffffffff
    lo = (A0 & 0xffffffff) | ((A1 & 0xffffffff) << 32)
    hi = (A2 & 0xffffffff) | (r3 << 32)
    lo2 = (lo + add_lo) & M64
    hi = (hi + add_hi + (1 if lo2 < lo else 0)) & M64
    return hi, lo2


A1 = (0x9FCCF645, 0x4385DF64, 0x1FC65DA4, 0x2360ED05)       # the limbs pcg64.hpp multiplies by, low first
A4, G4 = (0x42D45771, 0xD194DFBE, 0x27DB7A9B, 0xF4DD4173), (0xADEFBA1C, 0x817FA187, 0x4B07E063, 0x610E11A1)
A16, G16 = (0x288C03C1, 0xF6EF6D3D, 0x3B315F84, 0xB6A4239F), (0x352439F0, 0xA9072151, 0x168FB143, 0x6ED699DB)


def column_step(s_hi, s_lo, inc_hi, inc_lo):
    return column_mul_add(s_hi, s_lo, A1, inc_lo, inc_hi)


def limbs(m):
    return sum(x << (32 * i) for i, x in enumerate(m))


def test_jump_ahead_constants_are_powers_of_the_step():
    a = forge.MULT
    assert limbs(A1) == a
    for n, an, gn in ((4, A4, G4), (16, A16, G16)):
        assert limbs(an) == pow(a, n, 1 << 128)
        assert limbs(gn) == sum(pow(a, i, 1 << 128) for i in range(n)) % (1 << 128)


@pytest.mark.parametrize("k", (3, 6, 7, 70, 150))
@pytest.mark.parametrize("case", CASES)
def test_device_step_restatements_on_forged_records(k, case):
    """The scalar (Pcg64U) and the column (Pcg64) form of the step under the bounded draw, on the forged records; the 4- and
    16-step jumps land where stepping does from the very states the forged draws leave."""
    rec, expect = forge.tie_case_record(case, k)
    gen = generator_from(rec)
    want = int(gen.integers(0, k))
    for name, fn in (("scalar", scalar_step), ("column", column_step)):
        pred = forge.Stream(rec, next64=fn)
        assert pred.below(k) == want and pred.record() == after(gen) and pred.rejections == expect, (name, case, k)
    hi, lo, ihi, ilo = after(gen)[:4]
    assert scalar_output(hi, lo) == forge.output((hi << 64) | lo)
    for n, an, gn in ((4, A4, G4), (16, A16, G16)):
        g_hi, g_lo = column_mul_add(ihi, ilo, gn, 0, 0)           # inc_g4 / inc_g16: inc * G_n
        j_hi, j_lo = column_mul_add(hi, lo, an, g_lo, g_hi)       # advance4 / advance16
        s = (hi << 64) | lo
        for _ in range(n):
            s = forge.step(s, (ihi << 64) | ilo)
        assert (j_hi << 64) | j_lo == s, n


# ---- the planner restatements, through the generators they take ----------------------------------------------------------------
def same(a, b):
    assert set(a) == set(b)
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=np.asarray(x).dtype.kind == "f"), key
        else:
            assert x == y, key


@pytest.mark.parametrize("k,n_actions", [(3, 3), (3, 5), (6, 6), (7, 8), (70, 70), (150, 150)])
@pytest.mark.parametrize("case", CASES)
def test_olop_restatement_meets_the_forged_rejections(k, n_actions, case):
    """OLOP draws its episode's seed (one word) and then the uniform continuation among the k listed actions: lead = 1."""
    t, r, term, avail = zero_table(12, n_actions, k)
    rec, expect = forge.tie_case_record(case, k, lead=1)
    thr = olr.thresholds("4*np.log(time)", "global", 4)
    gen, pred = generator_from(rec), forge.Stream(rec)
    a = olr.olop_plan(t, r, term, 0, 4, 3, 0.8, True, thr, "uniform", gen, available=avail)
    b = olr.olop_plan(t, r, term, 0, 4, 3, 0.8, True, thr, "uniform", pred, available=avail)
    same(a, b)
    assert after(gen) == pred.record()
    assert pred.rejections >= expect and (expect == 0 or a["error"] is None)


@pytest.mark.parametrize("k", (3, 6, 7, 70, 150))
@pytest.mark.parametrize("case", CASES)
def test_brue_restatement_meets_the_forged_rejections(k, case):
    """BRUE draws a rollout's seed (one word) and then every action with integers(A): lead = 1, k = A."""
    t, r, term, _ = zero_table(12, k, k)
    rec, expect = forge.tie_case_record(case, k, lead=1)
    gen, pred = generator_from(rec), forge.Stream(rec)
    a = brr.brue_plan("deterministic", t, r, term, 0, 12, 3, 0.9, gen)
    b = brr.brue_plan("deterministic", t, r, term, 0, 12, 3, 0.9, pred)
    same(a, b)
    assert after(gen) == pred.record() and pred.rejections >= expect


@pytest.mark.parametrize("k,n_actions", [(3, 3), (3, 5), (6, 6), (7, 8), (70, 70), (150, 150)])
@pytest.mark.parametrize("case", CASES)
def test_gbopd_restatement_meets_the_forged_rejections(k, n_actions, case):
    """GBOP-D's first draw is the sampling rule's tie among the root's k listed actions (second run): lead = 0."""
    t, r, _, avail = zero_table(12, n_actions, k)
    rec, expect = forge.tie_case_record(case, k)
    out = []
    for g in (generator_from(rec), forge.Stream(rec)):
        graph = gbr.Graph(t, r, 0.9, available=avail)
        plan = graph.plan(0, 4 * n_actions, 1e-2, 5, g)
        out.append((plan, graph.listing(), g))
    assert out[0][0] == out[1][0] and not gbr.same_listing(out[0][1], out[1][1])
    assert after(out[0][2]) == out[1][2].record() and out[1][2].rejections >= expect


@pytest.mark.parametrize("k,masked", [(k, False) for k in (3, 6, 7, 70, 150)] + [(70, True), (150, True)])
def test_gape_restatement_meets_the_forged_continuation_draws(k, masked):
    """MDP-GapE draws its episode's seed (one word) and then, at the childless node below the root, integers(k) over the k
    environment actions: lead = 1.  Every record of the batch the GPU test plans: numpy's Generator against the prediction."""
    from tests import gape_cases as gc
    case, names = gc.forged_continuation_case(k, masked)
    unlisted = 0
    for i, (s0, rec) in enumerate(zip(case["roots"], case["rng"])):
        res, rng_after, seen = gc.restate_plan(case, s0, rec)
        words, arg, rejections = gc.first_tie(case, s0, rec)
        assert (words, arg) == (1, k), i
        if names[i] != "seeded":
            assert rejections == forge.tie_case_record(names[i], k, salt=i // 6, lead=1)[1], (i, names[i])
        pred = forge.Stream(rec)
        pred.below(1 << 30)
        action, listed, column = [v for kind, v in seen if kind == "continuation"][0]
        below_root = res["state"][1 + int(case["available"][s0].sum())]     # the first decision node made after the root's arms
        assert action == column == pred.below(k) and listed == bool(case["available"][below_root, int(action)]), i
        unlisted += not listed
        assert res["error"] is None and gc.margin(seen) > gc.MARGIN, i
    assert {n for n in names} == set(forge.TIE_CASES) - {"reject3"} and (unlisted >= 8) == masked


@pytest.mark.parametrize("m", (3, 6, 7, 70, 150))
def test_gape_restatement_meets_the_forged_tie_draws(m):
    """With continuation "zeros" the first draw that is no seed draw is random_argmax among the m unvisited children of the node
    below the root that is visited twice: three seed words come before it (skip = 1 output, lead = 1 word), whatever they are."""
    from tests import gape_cases as gc
    case, names, words = gc.forged_tie_case(m)
    assert words == 3
    met = set()
    for i, (s0, rec) in enumerate(zip(case["roots"], case["rng"])):
        res, rng_after, seen = gc.restate_plan(case, s0, rec)
        assert gc.first_tie(case, s0, rec)[:2] == (3, m), i
        size, rank, position = [v for kind, v in seen if kind == "ties" and v[0] > 1][0]
        pred = forge.Stream(rec)
        for _ in range(3):
            pred.below(1 << 30)
        assert size == m and rank == pred.below(m) and position == rank + 1, i      # (the visited child is the first one)
        if names[i] != "seeded":
            assert pred.rejections == forge.tie_case_record(names[i], m, salt=i // 6, lead=1)[1], (i, names[i])
        met.add(pred.rejections)
        assert res["error"] is None and gc.margin(seen) > gc.MARGIN, i
    assert met >= {0, 1, 2}


# ---- where the GPU tests put the forged draw -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 6, 7, 70, 150))
@pytest.mark.parametrize("case", CASES)
def test_oracle_uct_meets_the_forged_tie_after_the_first_rollout(k, case):
    """Episode 1 of MCTS expands the root and draws H rollout actions; episode 2 starts with the tie among the k children.
    tests/test_gpu_forged_draws.py forges that draw with skip = H: the oracle's record after two episodes is the predicted one."""
    horizon = 6
    t, r, term, _ = zero_table(12, k, k)
    rec, expect = forge.tie_case_record(case, k, skip=horizon)
    p = np.ones(k) / k
    pred = forge.Stream(rec)
    for _ in range(horizon):
        pred.random()
    one = oracle.uct_plan(t, r, term, 0, 1, horizon, 0.9, 5.0, p, p, rec)
    assert [int(x) for x in one["rng_after"]] == pred.record()
    pick = pred.below(k)
    assert pred.rejections == expect
    for _ in range(horizon - 1):
        pred.random()
    two = oracle.uct_plan(t, r, term, 0, 2, horizon, 0.9, 5.0, p, p, rec)
    assert [int(x) for x in two["rng_after"]] == pred.record()
    assert two["tree"]["count"][1:1 + k].tolist() == [int(j == pick) for j in range(k)]


@pytest.mark.parametrize("k,n_actions", [(3, 8), (6, 8), (7, 8), (70, 70), (150, 150)])
@pytest.mark.parametrize("case", CASES)
def test_oracle_optimistic_planners_meet_the_forged_tie_first(k, n_actions, case):
    """OPD, robust OPD and state-aware OPD draw only in get_plan: the first draw is the tie among the root's k listed children."""
    t, r, term, avail = zero_table(12, n_actions, k)
    rec, expect = forge.tie_case_record(case, k)
    pred = forge.Stream(rec)
    pick = pred.below(k)
    assert pred.rejections == expect
    budget = 3 * n_actions
    assert int(oracle.opd_plan(t, r, term, 0, budget, 0.8, rng_state=rec, available=avail)["plan"][0]) == pick
    tm, rm, av = np.stack([t, (t + 3) % 12]), np.stack([r, r]), np.stack([avail, avail])
    assert int(oracle.ropd_plan(tm, rm, None, 0, budget, 0.8, rng_state=rec, available=av)["plan"][0]) == pick
    # state-aware OPD descends twice per plan and returns the second descent (state_aware.py:122-127): both are walked here
    # over the oracle's own tree with the predicted stream -- the forged tie is the first descent's first draw
    sa = oracle.saopd_plan(t, r, term, 0, budget, 0.8, rng_state=rec, available=avail, max_plan_len=budget + 1)
    tree, walk = sa["tree"], forge.Stream(rec)
    for _ in range(2):
        node, plan = 0, []
        while tree["first_child"][node] >= 0:
            fc, nc = int(tree["first_child"][node]), int(tree["n_children"][node])
            low = tree["lower"][fc:fc + nc]
            ties = np.flatnonzero(low == low.max())
            if node == 0:
                assert len(ties) == k
            node = fc + int(ties[walk.below(len(ties))])
            plan.append(int(tree["action"][node]))
    assert plan == sa["plan"].tolist() and [int(x) for x in sa["rng_after"]] == walk.record()
    assert walk.rejections >= expect


@pytest.mark.parametrize("kind,closed", [("stochastic", False), ("sparse", True)])
@pytest.mark.parametrize("k", (3, 6, 7, 70, 150))
@pytest.mark.parametrize("case", CASES)
def test_oracle_stochastic_uct_meets_the_forged_tie_after_the_first_rollout(kind, closed, k, case):
    """MCTS on a stochastic model draws its env steps from the ENV generator's clone: the planner's generator gives H rollout
    draws in episode 1, then episode 2's tie among the k children -- where the GPU test forges it (skip = H)."""
    horizon = 6
    cfg = stochastic_model(kind, 12, k, zero_rewards=True)
    rec, expect = forge.tie_case_record(case, k, skip=horizon)
    erng = forge.tie_case_record("seeded", k, salt=5)[0]
    p = np.ones(k) / k
    pred = forge.Stream(rec)
    for _ in range(horizon):
        pred.random()

    def after_episodes(n):
        out = oracle.uct_plan_stoch(cfg["mode"], cfg["transition"], cfg["reward"], None, 0, n, horizon, 0.9, 5.0, p, p, rec, erng,
                                    next_states=cfg["next"], closed_loop=closed)
        return [int(x) for x in out["rng_after"]]
    assert after_episodes(1) == pred.record()
    pred.below(k)
    assert pred.rejections == expect
    for _ in range(horizon - 1):
        pred.random()
    assert after_episodes(2) == pred.record()


# ---- models forged to a clone's draw (tests/forged_clone_cases.py) ---------------------------------------------------------------
TWIN_SETS = [("stochastic", fc.DENSE_W, "word", 0), ("stochastic", fc.DENSE_W, "word", 1), ("stochastic", fc.DENSE_W, "zeros", 0)] + \
            [("sparse", B, first, 0) for B in (1, 3, 4, 5) for first in ("word", "zeros")] + [("sparse", 4, "word", 1)]
N_ACTIONS = 3


def clone_of(x):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(x))))


def test_clone_k53_is_numpys_own_draw():
    for x in (0, 1, 2 ** 30 - 1, 123456789, 0x9E3779B9 >> 2):
        u = clone_of(x).random(3)
        raw = np.random.PCG64(np.random.SeedSequence(x)).random_raw(3)
        for n in range(3):
            k = forge.clone_k53(x, n)
            assert k * 2.0 ** -53 == u[n] and k == int(raw[n]) >> 11


def assert_twin_on_numpy(x, n, row, b, twin, want):
    """The forged row on numpy itself: exact cumsum, choice() of the clone's n-th draw, and 'left' against 'right'."""
    W = len(row)
    ints = [int(v * 2.0 ** 53) for v in row]
    assert all(v >= 0 for v in ints) and sum(ints) == forge.TWO53
    cdf = row.cumsum()
    assert cdf[-1] == 1.0 and [int(c * 2.0 ** 53) for c in cdf] == list(np.cumsum(np.array(ints, dtype=object)))
    k53 = forge.clone_k53(x, n)
    assert sum(ints[:b + 1]) == k53 + twin
    gen = clone_of(x)
    gen.random(n)
    assert int(gen.choice(W, p=row)) == want == (b if twin else forge.passed(row, b))
    u = k53 * 2.0 ** -53
    right, left = int(np.searchsorted(cdf, u, "right")), int(np.searchsorted(cdf, u, "left"))
    assert right == want and left == b
    assert (left != right) == (twin == 0)          # the pair tells `<` from `<=`: only the twin ON the threshold moves
    # the form the kernels search in: integer thresholds ceil(cdf * 2^53) <= k
    assert sum(forge.threshold53(c) <= k53 for c in cdf) == want
    assert sum(forge.threshold53(c) < k53 for c in cdf) == b


@pytest.mark.parametrize("kind,W,first,step", TWIN_SETS)
def test_clone_twins_on_numpy(kind, W, first, step):
    batch = fc.clone_twins(kind, W, N_ACTIONS, first=first, step=step)
    seen = set()
    for c in batch["cases"]:
        if c["b"] is None:
            continue
        assert np.array_equal(batch["cfg"]["transition"][c["state"], c["action"]], c["row"])
        assert_twin_on_numpy(c["x"], step, c["row"], c["b"], c["twin"], c["want"])
        seen.add((c["x"], c["b"], c["twin"]))
    bs = fc.DENSE_BS if kind == "stochastic" else fc.SPARSE_BS[W]
    assert seen == {(w >> 2, b, t) for w in fc.SEED_WORDS for b in bs for t in (0, 1)}
    assert {w >> 2 for w in fc.SEED_WORDS} >= {0, 1, 2 ** 30 - 1}
    if len(bs) > 1:
        assert any((c["row"] == 0).any() for c in batch["cases"])         # rows with equal adjacent thresholds


def next_state(cfg, s, a, idx):
    return int(idx) if cfg["mode"] == "stochastic" else int(cfg["next"][s, a, idx])


@pytest.mark.parametrize("kind,W,first,step", [t for t in TWIN_SETS if t[2] == "word"])
def test_brue_restatement_meets_the_forged_rows(kind, W, first, step):
    """The rollout's seed is the record's first word, its first action the second, and the clone's draw number ``step`` meets
    the forged row: the tree's first (second) outcome node is the state numpy's choice gives."""
    batch = fc.clone_twins(kind, W, N_ACTIONS, first=first, step=step)
    cfg = batch["cfg"]
    for c in batch["cases"]:
        i = c["root"]
        st = forge.LoggingStream(batch["records"][i])
        res = brr.brue_plan(cfg["mode"], cfg["transition"], cfg["reward"], np.zeros(len(cfg["reward"]), bool), i, 12, 3, 0.9, st,
                            nxt=cfg["next"])
        assert st.log[0][:4] == ("below", 0, 0, 1 << 30) and st.log[1][:4] == ("below", 1, 1, N_ACTIONS)
        assert st.log[0][4] == st.log[1][4] == 0
        assert forge.Stream(batch["records"][i]).below(1 << 30) == c["x"]
        if c["b"] is None:
            continue
        # creation order: chance node 1, outcome 2 (step 0); chance node 3, outcome 4 (step 1)
        node = 2 + 2 * step
        assert res["key"][node - 1] == c["action"] and res["key"][node] == next_state(cfg, c["state"], c["action"], c["want"])
        assert res["key"][node] != next_state(cfg, c["state"], c["action"], c["b"]) or c["twin"] == 1
        if step == 1:
            assert res["key"][2] == c["state"]


@pytest.mark.parametrize("kind,W,first,step", [t for t in TWIN_SETS if t[3] == 0])
def test_olop_stoch_restatement_meets_the_forged_rows(kind, W, first, step):
    """One episode of two steps: the seed is the record's first word, the uniform continuation the second ("zeros": none), and the
    second step's reward is that of the state the forged row gives -- the tree holds no states, the rewards tell."""
    batch = fc.clone_twins(kind, W, N_ACTIONS, first=first, step=0)
    cfg = batch["cfg"]
    thr = olr.thresholds("4*np.log(time)", "global", 1)
    for c in batch["cases"]:
        i = c["root"]
        st = forge.LoggingStream(batch["records"][i])
        res = osr.olop_stoch_plan(cfg["mode"], cfg["transition"], cfg["reward"], None, i, 1, 2, 0.8, True, thr,
                                  "uniform" if first == "word" else "zeros", st, next_states=cfg["next"])
        assert res["error"] is None and st.log[0][:4] == ("below", 0, 0, 1 << 30)
        if first == "word":
            assert st.log[1][:4] == ("below", 1, 1, N_ACTIONS) and st.log[1][4] == 0
        else:
            assert len(st.log) == 1
        path = [n for n in range(len(res["count"])) if res["count"][n] == 1]
        assert len(path) == 2 and res["action"][path[0]] == c["action"] and res["depth"][path[1]] == 2
        if c["b"] is None:
            continue
        a2 = int(res["action"][path[1]])
        assert res["cum"][path[1]] == cfg["reward"][next_state(cfg, i, c["action"], c["want"]), a2]
        if c["twin"] == 0:
            assert res["cum"][path[1]] != cfg["reward"][next_state(cfg, i, c["action"], c["b"]), a2]


@pytest.mark.parametrize("k", fc.TIE_KS)
def test_olop_stoch_restatement_meets_the_forged_rejections(k):
    """On a one-hot model the restatement draws what olop_restatement draws on the table: seed word, then the tie (lead = 1)."""
    n_actions = 8 if k < 8 else k
    cfg, (t, r, term), avail = fc.one_hot_tie_model(12, n_actions, k)
    thr = olr.thresholds("4*np.log(time)", "global", 4)
    for case in [c for c in CASES if c != "reject3"]:
        rec, expect = forge.tie_case_record(case, k, lead=1)
        st = forge.LoggingStream(rec)
        a = osr.olop_stoch_plan("stochastic", cfg["transition"], cfg["reward"], None, 0, 4, 3, 0.8, True, thr, "uniform", st,
                                available=avail)
        b = olr.olop_plan(t, r, term, 0, 4, 3, 0.8, True, thr, "uniform", forge.Stream(rec), available=avail)
        assert st.log[1][:2] == ("below", 1) and st.log[1][3:] == (k, expect), case
        for key in ("plan", "parent", "action", "count", "cum", "mu", "vu"):
            assert np.array_equal(a[key], b[key]), (case, key)


# ---- Sparse Sampling: the clone of one sample, and the root's tie -----------------------------------------------------------------
SS_SETS = [("stochastic", 150, 1), ("sparse", 2, 1), ("sparse", 3, 1), ("stochastic", 2, 1), ("stochastic", 3, 1), ("sparse", 3, 2)]


def ss_counts(cfg, s0, horizon, rec, action):
    """Outcome counts {state: count} of the root's chance node of ``action``, and the stream after the plan."""
    st = forge.LoggingStream(rec)
    res = ssr.ss_plan(cfg["mode"], cfg["transition"], cfg["reward"], s0, horizon, fc.SS_C, 0.9, st, nxt=cfg["next"])
    chance = [n for n in range(len(res["parent"])) if res["parent"][n] == 0 and res["key"][n] == action]
    assert len(chance) == 1
    kids = [n for n in range(len(res["parent"])) if res["parent"][n] == chance[0]]
    return {int(res["key"][n]): int(res["count"][n]) for n in kids}, st


@pytest.mark.parametrize("kind,W,horizon", SS_SETS)
def test_sparse_sampling_twins_on_numpy_and_the_sample_that_meets_them(kind, W, horizon):
    """Every case: the target sample's word is the forged one, its clone's draw sits on / below cdf[b] of the row, and in the
    restatement exactly that ONE sample changes sides when the row is swapped for its twin."""
    batches = fc.ss_batches(kind, W, horizon)
    assert sum(len(b["cases"]) for b in batches) == len(fc.ss_cases(W, horizon))
    swapped = 0
    for batch in batches:
        cfg = batch["cfg"]
        for c in batch["cases"]:
            rec = batch["records"][c["root"]]
            words = ssr.half_words(rec, c["t"] + 1)
            assert words[c["t"]] >> 2 == c["x"] and words[c["t"]] in fc.SS_WORDS and bool(rec[4]) == c["buffered"]
            assert np.array_equal(cfg["transition"][c["root"], c["action"]], c["row"])
            assert_twin_on_numpy(c["x"], 0, c["row"], c["b"], c["twin"], c["want"])
            if c["twin"] or (kind == "stochastic" and W < 150) or (c["b"] not in (0, W - 2) and c["t"] not in (0, 64)):
                continue                  # (the swap below: every on-twin of the small rows once, the wide rows' edges)
            got, st = ss_counts(cfg, c["root"], horizon, rec, c["action"])
            assert [e[:4] for e in st.log[:c["t"] + 1]] == [("below", j, (j + 1 - int(c["buffered"])) // 2, 1 << 30) for j in range(c["t"] + 1)]
            other = dict(cfg, transition=cfg["transition"].copy())
            other["transition"][c["root"], c["action"]] = forge.row_on(forge.clone_k53(c["x"]) + 1, W, c["b"],
                                                                        [j for j in range(W) if c["row"][j] == 0])
            base, _ = ss_counts(other, c["root"], horizon, rec, c["action"])
            hit, miss = next_state(cfg, c["root"], c["action"], c["want"]), next_state(cfg, c["root"], c["action"], c["b"])
            moved = dict(base)
            moved[miss] = moved.get(miss, 0) - 1
            moved[hit] = moved.get(hit, 0) + 1
            assert {s: n for s, n in moved.items() if n} == got, (c["t"], c["b"])
            swapped += 1
    assert swapped >= 8 or (kind == "stochastic" and W < 150)


@pytest.mark.parametrize("k", fc.TIE_KS)
def test_sparse_sampling_restatement_meets_the_forged_root_tie(k):
    """Horizon 1 on a zero-reward table: the samples consume k * C words whatever they are, then the root ties among its k
    listed actions -- the LAST draw of the plan, where the record's forged words sit."""
    from tests.helpers import zero_table
    n_actions = 8 if k < 8 else k
    t, r, _, avail = zero_table(12, n_actions, k)
    n_words = k * fc.SS_TIE_C
    recs, names, expect = fc.ss_tie_batch(k, 2 * len(fc.SS_TIE_CASES), n_words)
    assert set(names) == set(forge.TIE_CASES) - {"reject3"}
    for rec, name, e in zip(recs, names, expect):
        st = forge.LoggingStream(rec)
        res = ssr.ss_plan("deterministic", t, r, 0, 1, fc.SS_TIE_C, 0.9, st, available=avail if k < n_actions else None)
        assert res["samples"] == n_words and len(st.log) == n_words + 1
        assert st.log[-1][0] == "below" and st.log[-1][1] == n_words and st.log[-1][3] == k, name
        if e is not None:
            assert st.log[-1][4] == e, (name, k)
        if name == "buffered_plain" and n_words % 2 == 0:
            assert st.log[-1][2] == st.outputs                       # the tie's word came from the buffered half: no new output
    if k & (k - 1):
        assert max(e for e in expect if e is not None) == 2


# ---- BRUE's estimate() choice on an exact boundary --------------------------------------------------------------------------------
def test_brue_estimate_choice_is_the_sixth_output_over_counts_one_one():
    cfg = fc.estimate_chain()
    recs, ks = fc.estimate_records()
    values = []
    for rec, k53 in zip(recs, ks):
        st = forge.LoggingStream(rec)
        res = brr.brue_plan("stochastic", cfg["transition"], cfg["reward"], np.zeros(6, bool), 0, fc.EST["budget"], fc.EST["horizon"],
                            fc.EST["gamma"], st)
        choices = [e for e in st.log if e[0] == "choice"]
        assert len(choices) == 6 and st.outputs == 7 and res["env_steps"] == 6
        target = choices[4]
        assert target[2] == fc.EST["skip"] and target[3].tolist() == [0.5, 0.5]      # counts (1, 1) / 2
        assert sorted(fc.estimate_sides(rec)) == [2, 3]
        replay = forge.Stream(rec)
        replay.below(1 << 30)
        for _ in range(3):
            replay.random()
        replay.below(1 << 30)
        replay.random()
        assert replay.random() == k53 * 2.0 ** -53
        assert int(np.searchsorted([0.5, 1.0], k53 * 2.0 ** -53, "right")) == (1 if k53 == 1 << 52 else 0)
        assert int(np.searchsorted([0.5, 1.0], k53 * 2.0 ** -53, "left")) == 0
        values.append(float(res["stat"][1]))
    for on, below in zip(values[0::2], values[1::2]):
        assert on != below              # the root's chance value holds R(3) = 0.75 or R(2) = 0.25 of the chosen outcome
