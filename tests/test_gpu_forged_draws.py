"""Forged generator records on the device: the draws no seed reaches (tests/forge.py; tests/test_forge_host.py ties the same
records to numpy, the oracle and the restatements, and pins where each oracle planner meets the forged draw).  Every comparison
is on bits, against the reference each planner's own test uses -- plan, tree or listing, and the generator record after the
plan -- with ONE exception inherited from tests/test_gpu_olop.py: OLOP's mu / value_upper and root value within 1e-12 (the
device's log in the KL bound); its plans, trees, counts and generator records are exact.

TIE DRAWS.  Tables whose rewards are all zero: a planner's first decision is a tie among exactly the k listed actions, and
the batch gives every root another record -- forge.TIE_CASES: 0, 1, 2 and 3 rejected words (3 = buffered word, low half, high
half), a word whose leftover sits ON Lemire's threshold (it enters the bounded draw's ``if`` and skips its loop), an ordinary
word from the buffer, and a seeded control -- so the lanes of a wave part ways inside the rejection loop.
k in {3, 6, 7, 70, 150} for every planner (150: three chunks of the tie draw over more than 64 lanes, a full one in the
middle); a masked table where k < |A|.

  planner / form                                                                    k                     forged draw
  UCT uct_global, uct_global_spill, uct_ldsr, uct_quad, uct_row_shared (2 and 4
      roots per wave), uct_lone, uct_lone_mw (1, 4, 8 waves)                        3, 6, 7               2nd episode's root tie
  UCT uct_global, the generic many-actions kernel (the forms above plan 2 .. 8
      actions: 70 and 150 can only run here)                                        70, 150               (after H outputs)
  UCT uct_policy: per-state tables, packed records (|A| <= 5: k = 3), listed,
      listed + ordered (2 .. 8 actions: mp_uct_plan_policy refuses more)            3, 6, 7 (|A| = k, 8)  same
  UCT one model per root: uct_lone_each, uct_row_each, uct_global / uct_global      3, 6, 7 / 70, 150     same
  UCT uct_cartpole, replicas of 64 (the default at this batch), 16, 4 and 1 lanes   2 (never rejects)     buffered half on entry only
  mp_uct_plan_stochastic open / closed loop, dense / sparse                         3, 6, 7, 70, 150      2nd episode's root tie
  OPD opd_lds, opd_ldsx, opd_wide_sib_small, opd_wide_cls_small / opd_any;
      mp_opd_plan_models (opd_lds / opd_any)                                        3, 6, 7 / 3, 70, 150  the plan's first choice
  robust OPD ropd_lds_m2 / ropd_any                                                 3, 6, 7 / 70, 150     the plan's first choice
  state-aware OPD saopd_lane; "wave": saopd_wave_lds (three expansions leave the
      LDS dictionaries no use, 28 planners take the arena to LDS)                   3, 6, 7, 70, 150      the plan's first choice
      / saopd_lane (more actions than lanes, whatever the mapping asked for)        (wave: 70, 150)
      saopd_wave ("wave-plain"), saopd_wave_dict ("wave-dict": 13 expansions;
      saopd_wave_dict_retry at k = 6 and 7, whose backups fill the queue once)      3, 6, 7               the plan's first choice
  OLOP (uniform continuation)                                                       3, 6, 7, 70, 150      first continuation draw (after
                                                                                                          the episode's seed word)
  BRUE (the rollout's integers(|A|))                                                3, 6, 7, 70, 150      first action draw (same)
  GBOP-D                                                                            3, 6, 7, 70, 150      the sampling rule's first tie
  MDP-GapE (uniform continuation over k = |A| environment actions; at 70 and 150
      also under a mask that leaves the forged values unlisted: rank 0)             3, 6, 7, 70, 150      first continuation draw (same)
  MDP-GapE (continuation "zeros": random_argmax among the m unvisited children
      of the first node below the root that is visited twice)                       m = 3, 6, 7, 70, 150  the plan's first tie draw (after
                                                                                                          three seed words: skip 1, lead 1)
  in tests/test_gpu_forged_clone_draws.py:
  stochastic OLOP olop_stoch_dense (one-hot rows, uniform continuation)             3, 6, 7, 70, 150      first continuation draw (after
                                                                                                          the episode's seed word)
  Sparse Sampling ss_wave_lds; one model per root ss_each_lds / ss_each_global      3, 6, 7, 70, 150      the root's tie, the plan's LAST
                                                                                    / 3, 6, 7             draw (after k * C sample words)

The form is asserted by name in every test: mp_uct_plan_stochastic runs uct_stoch_r0 (dense rows), r4 (sparse rows of 3 and 4),
r1 / r2 (sparse rows of 2: compact records / kept at 32 bytes) with 16-bit path entries; these small batches run olop_global,
brue_global and gbopd_wave_lds.  SKIPPED_FORMS lists what could not be selected at these shapes.

The quad, row and CartPole forms share generator work by jump-ahead: reject3 and buffered_plain hand them has_uint32 = 1.
(OLOP and BRUE draw a seed word first, which leaves room for two forged rejections: their batches hold no reject3.)

EXACT CDF BOUNDARIES.  The forged random() is k53 * 2^-53 with k53 = t and t - 1 for every threshold
t = ceil(cdf[a] * 2^53) of the row it is compared with (low 11 bits all zeros and all ones), as the plan's first draw on: the
state-independent UCT forms above and CartPole (uniform rows of 2, 3, 5, 8, 9 actions; a row with a zero in the middle and
trailing zeros); the rollout rows of uct_stoch.hip, and its model rows through the env generator's record (every episode's
clone starts from it); mp_env_step_stochastic on dense rows of 150 entries and sparse rows of 1, 3, 4, 5 successors, where
the expected state is numpy.searchsorted(cdf, u, 'right') itself.  The per-state-policy forms (fused 32-byte records with the
shipped 32 coarse bits, packed 16-byte ones with 10; listed and ordered policies) get them as the first draw -- decided by the
root's exact row, coarsened in the kernel -- AND as the second, decided by the thresholds stored in the record the walk
fetched; there also t + 1 and both ends of the range that shares the threshold's coarse bits.

REACHED BY FORGING THE MODEL (tests/test_gpu_forged_clone_draws.py; no caller-passed record holds these draws, but the record
fixes the seed x of the clone a planner seeds on the device (seed_sequence.hpp), numpy gives the clone's draws, and the model
row they meet is built so that the draw sits on, or one step below, a cdf entry): the model-row draws of BRUE's per-rollout
clone (ballot search, dense rows of 150 and sparse rows of 1, 3, 4, 5; first and second step), of olop_stoch_kernel's per-episode
clone (the same search, continuation "zeros" and "uniform") and of one chosen sample of Sparse Sampling's root (binary search
on the sample's own lane, the jump to its half-word with and without a half buffered on entry; both frame forms).  Reached
with ``skip``, where the number of outputs before the draw does not depend on their values: Sparse Sampling's root tie (table
above) and BRUE's estimate() draw, choice(p=counts / counts.sum()), at u == cdf[0] over counts (1, 1) on a one-action chain.

OUT OF REACH: OLOP's, BRUE's, Sparse Sampling's and UCT's env seed draws are powers of two (2^30) and cannot reject; BRUE's final
root tie, and every later tie of a plan whose draw count depends on the drawn values (a rollout that may end early, a tree
whose shape the draws decide), are met only with unforged words; BRUE's estimate() choice over more than 64 outcomes (the
chunk logic of the kernel's weighted choice) meets an exact cdf entry in no plan a test can construct."""
import numpy as np
import pytest

from tests import forge
from tests.helpers import CDF_ROWS as ROWS
from tests.helpers import assert_form, bfs_by_parent, generator_from, stochastic_model, uct_stoch_form, value_table, zero_table

pytestmark = pytest.mark.gpu

SKIPPED_FORMS = []        # (form, reason): forms that no small shape selects -- none

S = 12
N_TIE = 4 * len(forge.TIE_CASES)          # 28 roots: every case with four different words / increments
UCT_KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_LONE_WAVES", "MP_UCT_EACH", "MP_UCT_ROW", "MP_UCT_ROWS",
             "MP_UCT_ROW_WAVES", "MP_UCT_ROW_ROOTS", "MP_UCT_PATH", "MP_UCT_LANES", "MP_UCT_LDSR_WAVES", "MP_UCT_CART_REP",
             "MP_UCT_CART_WAVES", "MP_UCT_POLICY_RECORD", "MP_UCT_COARSE_BITS", "MP_UCT_STOCH_FUSED", "MP_UCT_STOCH_GENERIC_A",
             "MP_OPD_MODEL", "MP_OPD_WIDE", "MP_SAOPD_MODEL", "MP_SAOPD_DICT", "MP_SAOPD_LDS")
UCT_TABLE_FORMS = [("uct_global", "MP_UCT_MODEL=global"), ("uct_global_spill", "MP_UCT_MODEL=global MP_UCT_PATH=spill"),
                   ("uct_ldsr", "MP_UCT_MODEL=ldsr"), ("uct_quad", "MP_UCT_QUAD=1"), ("uct_row_shared", "MP_UCT_ROWS=1"),
                   ("uct_row_shared", "MP_UCT_ROWS=1 MP_UCT_ROW_ROOTS=4 MP_UCT_ROW_WAVES=2"), ("uct_lone", ""),
                   ("uct_lone_mw", "MP_UCT_LONE_WAVES=1"), ("uct_lone_mw", "MP_UCT_LONE_WAVES=4"),
                   ("uct_lone_mw", "MP_UCT_LONE_WAVES=8")]
GAMMA, TEMPERATURE = 0.9, 5.0


@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    yield c
    c.close()


def set_knobs(monkeypatch, knobs):
    for k in UCT_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in knobs.split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv(k, v)


def cdf_draws(p, coarse=()):
    """(k53, low11) around every threshold of the row: t - 1 and t with the dropped bits all zeros and all ones; with
    ``coarse`` (numbers of low bits a fused record drops) also t + 1 and both ends of the range sharing t's kept bits."""
    from oracle import oracle
    out, extra = [], set()
    for t in sorted({forge.threshold53(c) for c in oracle.policy_cdf(p)}):
        out += [(k, low) for k in (t - 1, t) for low in (0, 0x7ff)]
        for bits in coarse:
            m = (1 << bits) - 1
            extra |= {t + 1, t & ~m, t | m}
    out += [(k, 0x7ff * (i & 1)) for i, k in enumerate(sorted(extra))]
    return [(k, low) for k, low in dict.fromkeys(out) if 0 <= k < (1 << 53)]


def cdf_records(draws, skip=0):
    """One record per draw whose (skip + 1)-th random() is the forged one; every other record enters with a buffered half."""
    recs = [forge.double_record((forge.DEFAULT_INC + 2 * i * 0x9E3779B97F4A7C15F39CC0605CEDC834) & forge.M128, k53, low11,
                                hi=(forge.DEFAULT_HI + i * 0x0400000000000001) & forge.M64,
                                buffered=0xC0FFEE00 + i if i & 1 else None, skip=skip) for i, (k53, low11) in enumerate(draws)]
    return np.array(recs, dtype=np.uint64)


def assert_uct_equal(out, ref, rng, n=None):
    for k in ("plans", "plan_len", "root_child_count", "env_steps"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.array_equal(out["root_value"], ref["root_value"])
    assert np.array_equal(out["root_child_value"], ref["root_child_value"])
    np.testing.assert_array_equal(rng, ref["rng_after"])


def check_uct(ctx, tab, s0, episodes, horizon, prior, rollout, rng, expect, trees=(), policy_of=None, lists=None):
    """One batch on the device against the oracle: results, generator records, and whole trees of ``trees``."""
    from oracle import oracle
    t, r, term = tab
    a = r.shape[1]
    model = ctx.load_table(t, r, term)
    policy = None if policy_of is None else policy_of(model)
    rng0, rng_ref = rng.copy(), rng.copy()
    ctx.uct_reset_tree()
    if policy is None:
        out = ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, prior, rollout, rng, max_plan_len=horizon)
    else:
        out = ctx.uct_plan(model, s0, episodes, horizon, GAMMA, TEMPERATURE, None, None, rng, max_plan_len=horizon, policy=policy)
    assert ctx.last_kernel_variant() == expect, ctx.last_kernel_variant()
    pp, rp = (prior, rollout) if lists is None else lists
    ref = oracle.uct_plan_batch(t, r, term, s0, episodes, horizon, GAMMA, TEMPERATURE, pp, rp, rng_ref, max_plan_len=horizon)
    assert_uct_equal(out, ref, rng)
    for root in trees:
        tree = ctx.uct_tree(root, 1 + episodes * a)
        one = oracle.uct_plan(t, r, term, int(s0[root]), episodes, horizon, GAMMA, TEMPERATURE, pp, rp, rng0[root],
                              max_plan_len=horizon)["tree"]
        keys = ("parent", "action", "count", "value", "first_child") if lists is None else ("count", "value")
        for k in keys:
            np.testing.assert_array_equal(tree[k], one[k], err_msg="tree[{}] of root {}".format(k, root))
    if policy is not None:
        policy.close()
    model.close()
    return out


def tie_roots():
    return (np.arange(N_TIE) * 5 % S).astype(np.int32)


def case_roots(names, *cases):
    return [i for i, c in enumerate(names) if c in cases][:3]


# ---- UCT: tie draws --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 6, 7])
@pytest.mark.parametrize("expect,knobs", UCT_TABLE_FORMS)
def test_uct_tie_draws_every_table_form(ctx, monkeypatch, expect, knobs, k):
    """Episode 1 expands the root and rolls out H steps (H outputs); episode 2's first draw is the tie among the k children."""
    set_knobs(monkeypatch, knobs)
    horizon = 18                                  # two rounds of the rows' sixteen draws, five of the quad's four
    t, r, term, _ = zero_table(S, k, k)
    rng, names = forge.tie_batch(k, N_TIE, skip=horizon)
    p = np.ones(k) / k
    check_uct(ctx, (t, r, term), tie_roots(), 5, horizon, p, p, rng, expect, trees=case_roots(names, "reject3", "reject2"))


@pytest.mark.parametrize("k", [70, 150])
def test_uct_tie_draws_generic_many_actions_kernel(ctx, monkeypatch, k):
    """More children than lanes: the tie draw runs over chunks of 64."""
    set_knobs(monkeypatch, "")
    t, r, term, _ = zero_table(S, k, k)
    rng, names = forge.tie_batch(k, N_TIE, skip=6)
    p = np.ones(k) / k
    check_uct(ctx, (t, r, term), tie_roots(), 4, 6, p, p, rng, "uct_global", trees=case_roots(names, "reject3"))


def listed_tables(avail, weights=None):
    k = avail.sum(axis=1)
    w = np.where(avail, 1.0, 0.0) if weights is None else np.where(avail, weights, 0.0)
    table = w / w.sum(axis=1, keepdims=True)
    lists = dict(actions=[[int(a) for a in np.flatnonzero(row)] for row in avail],
                 p=[table[s, np.flatnonzero(avail[s])] for s in range(len(avail))])
    assert (k >= 1).all()
    return table, lists


@pytest.mark.parametrize("form,k", [(f, k) for f in ("tables", "packed", "listed", "ordered") for k in (3, 6, 7)
                                    if f != "packed" or k <= 5])     # (the packed records hold at most five actions)
def test_uct_tie_draws_per_state_policy_forms(ctx, monkeypatch, form, k):
    """uct_policy: per-state tables over |A| = k (fused 32-byte records; the packed 16-byte ones where |A| <= 5), a listed
    policy over k of 8 actions, and a rollout policy that lists them in an order of its own."""
    set_knobs(monkeypatch, "MP_UCT_POLICY_RECORD=packed" if form == "packed" else "")
    horizon = 7
    n_actions = 8 if form in ("listed", "ordered") else k
    t, r, term, avail = zero_table(S, n_actions, k)
    rng, names = forge.tie_batch(k, N_TIE, skip=horizon)
    table, lists = listed_tables(avail)
    slots = None
    prior_lists = rollout_lists = lists
    if form == "ordered":
        g = np.random.Generator(np.random.PCG64(k))
        slots = np.stack([np.concatenate([g.permutation(k), np.arange(k, n_actions)]) for _ in range(S)]).astype(np.uint8)
        rollout_lists = dict(actions=[[int(a) for a in slots[s, :k]] for s in range(S)], p=[table[s, slots[s, :k]] for s in range(S)])

    def policy_of(model):
        if form in ("tables", "packed"):
            return ctx.load_policy(model, table, table)
        return ctx.load_policy(model, table, table, listed=avail, rollout_slots=slots)
    ref_policies = (table, table) if form in ("tables", "packed") else (prior_lists, rollout_lists)
    check_uct(ctx, (t, r, term), tie_roots(), 5, horizon, None, None, rng, "uct_policy", policy_of=policy_of, lists=ref_policies)


@pytest.mark.parametrize("expect,knobs,k", [(e, kn, k) for e, kn in (("uct_lone_each", ""), ("uct_row_each", "MP_UCT_ROW=1"),
                                                                    ("uct_global", "MP_UCT_EACH=0 MP_UCT_MODEL=global"))
                                            for k in (3, 6, 7)] +
                         [("uct_global", "", 70), ("uct_global", "", 150)])   # (the LDS forms plan 2 .. 8 actions)
def test_uct_tie_draws_one_model_per_root(ctx, monkeypatch, expect, knobs, k):
    from oracle import oracle
    set_knobs(monkeypatch, knobs)
    horizon, n_models = 18, 5
    t, r, term, _ = zero_table(S, k, k)
    tr = np.stack([(t + m) % S for m in range(n_models)])
    tr = np.where(tr == np.arange(S)[None, :, None], (tr + 1) % S, tr)         # (no self-loop: no table has a terminal state)
    rw, tm = np.zeros((n_models, S, k)), np.zeros((n_models, S), bool)
    model = ctx.load_table_batch(tr, rw, tm)
    mi = (np.arange(N_TIE) % n_models).astype(np.int32)
    rng, _ = forge.tie_batch(k, N_TIE, skip=horizon)
    rng_ref = rng.copy()
    p = np.ones(k) / k
    out = ctx.uct_plan(model, tie_roots(), 5, horizon, GAMMA, TEMPERATURE, p, p, rng, max_plan_len=horizon, model_index=mi)
    assert ctx.last_kernel_variant() == expect, ctx.last_kernel_variant()
    ref = oracle.uct_plan_each(tr, rw, tm, mi, tie_roots(), 5, horizon, GAMMA, TEMPERATURE, p, p, rng_ref, max_plan_len=horizon)
    assert_uct_equal(out, ref, rng)
    model.close()


@pytest.mark.parametrize("knobs", ["", "MP_UCT_CART_REP=4", "MP_UCT_CART_REP=2", "MP_UCT_CART_REP=0"])
def test_cartpole_buffered_half_on_entry_and_first_draw_on_the_boundary(ctx, monkeypatch, knobs):
    """Two actions never reject: what can go wrong is the buffered half carried across the replicas' jump-ahead (a 32-bit draw
    served from it consumes no output) and the first rollout draw on the threshold of the two-action row."""
    from oracle import oracle
    from rl_agents_amd.envs import CartPoleEnv
    set_knobs(monkeypatch, knobs)
    params = CartPoleEnv().cartpole_params()
    model = ctx.load_cartpole(params)
    roll = np.array([0.35, 0.65])
    draws = cdf_draws(roll) + cdf_draws(np.ones(2) / 2)
    rng = np.concatenate([cdf_records(draws), forge.tie_batch(2, N_TIE)[0]])
    n = len(rng)
    assert (rng[:, 4] == 1).sum() >= 10
    x0 = np.random.Generator(np.random.PCG64(3)).uniform(-0.08, 0.08, size=(n, 4))
    rng_ref = rng.copy()
    prior = np.array([0.5, 0.5])
    out = ctx.uct_plan(model, x0, 8, 20, GAMMA, TEMPERATURE, prior, roll, rng, max_plan_len=8)
    assert ctx.last_kernel_variant() == "uct_cartpole"
    ref = oracle.uct_plan_batch(None, None, None, x0, 8, 20, GAMMA, TEMPERATURE, prior, roll, rng_ref, max_plan_len=8, cartpole=params)
    assert_uct_equal(out, ref, rng)
    model.close()


# ---- UCT: the first random() on a threshold ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["uniform2", "uniform3", "uniform5", "uniform8", "zeros"])
@pytest.mark.parametrize("expect,knobs", UCT_TABLE_FORMS)
def test_uct_first_rollout_draw_on_every_threshold(ctx, monkeypatch, expect, knobs, row):
    set_knobs(monkeypatch, knobs)
    rollout = ROWS[row]
    a = len(rollout)
    draws = cdf_draws(rollout)
    rng = cdf_records(draws)
    s0 = (np.arange(len(draws)) * 5 % S).astype(np.int32)
    check_uct(ctx, value_table(S, a), s0, 4, 6, np.ones(a) / a, rollout, rng, expect, trees=(0, len(draws) - 1))


def test_uct_first_rollout_draw_on_every_threshold_generic_kernel(ctx, monkeypatch):
    """Nine actions: beyond the eight thresholds the kernels hold by value."""
    set_knobs(monkeypatch, "")
    rollout = ROWS["uniform9"]
    draws = cdf_draws(rollout)
    s0 = (np.arange(len(draws)) * 5 % S).astype(np.int32)
    check_uct(ctx, value_table(S, 9), s0, 4, 6, np.ones(9) / 9, rollout, cdf_records(draws), "uct_global", trees=(0, len(draws) - 1))


POLICY_ROWS = {"uniform2": ROWS["uniform2"], "uniform3": ROWS["uniform3"], "uniform5": ROWS["uniform5"], "uniform8": ROWS["uniform8"],
               "zeros": ROWS["zeros"], "skewed5": np.array([0.3, 0.0, 0.45, 0.25, 0.0])}


@pytest.mark.parametrize("step", ["first", "second"])
@pytest.mark.parametrize("record,row", [(rec, row) for rec in ("fused", "packed") for row in sorted(POLICY_ROWS)
                                        if rec != "packed" or len(POLICY_ROWS[row]) <= 5])    # (packed: at most five actions)
def test_uct_policy_records_decide_by_the_exact_row(ctx, monkeypatch, record, row, step):
    """The shipped coarse thresholds (32 bits in the fused records, 10 in the packed ones) and no knob: draws that share a
    threshold's coarse bits with the rest below, equal and above it are decided by the exact row.  The FIRST rollout step
    coarsens the root state's exact row itself; every later step compares with the thresholds stored in the record the walk
    fetched, so the forged draw is also made the SECOND one (one row for every state then: the state the first, unforged step
    leads to does not matter).  Whether the packed form was taken cannot be told from outside (the variant name is the same)."""
    rollout = POLICY_ROWS[row]
    a = len(rollout)
    set_knobs(monkeypatch, "MP_UCT_POLICY_RECORD=packed" if record == "packed" else "")
    other = np.roll(rollout, 1) if step == "first" else rollout     # odd states draw from another row: the records are per state
    draws = [(0, d) for d in cdf_draws(rollout, coarse=(21, 43))] + [(1, d) for d in cdf_draws(other, coarse=(21, 43))]
    s0 = np.array([(2 * i) % S + par for i, (par, _) in enumerate(draws)], dtype=np.int32)
    table = np.stack([rollout if s % 2 == 0 else other for s in range(S)])
    prior = np.full((S, a), 1.0 / a)
    for lo in range(0, len(draws), 64):
        part = slice(lo, lo + 64)
        recs = cdf_records([d for _, d in draws[part]], skip=0 if step == "first" else 1)
        check_uct(ctx, value_table(S, a), s0[part], 4, 6, None, None, recs, "uct_policy",
                  policy_of=lambda model: ctx.load_policy(model, prior, table), lists=(prior, table))


@pytest.mark.parametrize("step", ["first", "second"])
@pytest.mark.parametrize("form", ["listed", "ordered"])
def test_uct_listed_policies_first_draws_on_every_threshold(ctx, monkeypatch, form, step):
    """A policy over 5 listed of 8 actions, and a rollout policy that lists them in another order: the inverse CDF runs over the
    rollout policy's own listing.  One listing for every state, so that the second draw meets the same thresholds."""
    set_knobs(monkeypatch, "")
    n_actions, k = 8, 5
    t, r, term = value_table(S, n_actions)
    avail = np.zeros((S, n_actions), bool)
    avail[:, [0, 2, 3, 5, 6]] = True
    weights = np.tile(np.array([0.1, 0.0, 0.3, 0.2, 0.0, 0.25, 0.15, 0.0]), (S, 1))
    table, lists = listed_tables(avail, weights)
    slots, rollout_lists = None, lists
    if form == "ordered":
        order = [5, 0, 6, 3, 2, 1, 4, 7]
        slots = np.tile(np.array(order, np.uint8), (S, 1))
        rollout_lists = dict(actions=[order[:k]] * S, p=[table[s, order[:k]] for s in range(S)])
    draws = cdf_draws(rollout_lists["p"][0], coarse=(21, 43))
    s0 = (np.arange(len(draws)) * 5 % S).astype(np.int32)
    check_uct(ctx, (t, r, term), s0, 4, 6, None, None, cdf_records(draws, skip=0 if step == "first" else 1), "uct_policy",
              policy_of=lambda model: ctx.load_policy(model, table, table, listed=avail, rollout_slots=slots),
              lists=(lists, rollout_lists))


# ---- UCT on stochastic models ----------------------------------------------------------------------------------------------------
def same_parent_tree(tree, ref, keys):
    (oa, pa), (ob, pb) = bfs_by_parent(tree["parent"]), bfs_by_parent(ref["parent"])
    np.testing.assert_array_equal(pa, pb)
    for k in keys:
        assert np.array_equal(np.asarray(tree[k])[oa], np.asarray(ref[k])[ob]), k


def check_stochastic(ctx, cfg, s0, episodes, horizon, prior, rollout, rng, erng, closed, records, trees=()):
    """``records``: the form of the model's step records (tests.helpers.uct_stoch_form)."""
    from oracle import oracle
    if cfg["mode"] == "sparse":
        model = ctx.load_sparse(cfg["transition"], cfg["next"], cfg["reward"], None)
    else:
        model = ctx.load_dense(cfg["transition"], cfg["reward"], None)
    rng0, rng_ref = rng.copy(), rng.copy()
    mpl = (2 if closed else 1) * horizon
    out = ctx.uct_plan_stochastic(model, s0, episodes, horizon, GAMMA, TEMPERATURE, prior, rollout, rng, env_rng_state=erng,
                                  closed_loop=closed, max_plan_len=mpl)
    assert_form(ctx, uct_stoch_form(records, 16, len(prior)))
    ref = oracle.uct_plan_stoch_batch(cfg["mode"], cfg["transition"], cfg["reward"], None, s0, episodes, horizon, GAMMA, TEMPERATURE,
                                      prior, rollout, rng_ref, erng, next_states=cfg["next"], closed_loop=closed, max_plan_len=mpl)
    for k in ("plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.array_equal(out["root_value"], ref["root_value"])
    np.testing.assert_array_equal(rng, ref["rng_after"])
    for root in trees:
        one = oracle.uct_plan_stoch(cfg["mode"], cfg["transition"], cfg["reward"], None, int(s0[root]), episodes, horizon, GAMMA,
                                    TEMPERATURE, prior, rollout, rng0[root], erng[root], next_states=cfg["next"],
                                    closed_loop=closed, max_plan_len=mpl)["tree"]
        same_parent_tree(ctx.uct_stoch_tree(root), one, ("action", "is_obs", "count", "value"))
    model.close()


@pytest.mark.parametrize("k", [3, 6, 7, 70, 150])
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("kind", ["stochastic", "sparse"])
def test_stochastic_uct_tie_draws(ctx, monkeypatch, kind, closed, k):
    from rl_agents_amd import native
    set_knobs(monkeypatch, "")
    horizon = 6
    cfg = stochastic_model(kind, S, k, zero_rewards=True)
    rng, names = forge.tie_batch(k, N_TIE, skip=horizon)
    erng = native.seed_sequence_states((), 900 + k, N_TIE)
    p = np.ones(k) / k
    check_stochastic(ctx, cfg, tie_roots(), 5, horizon, p, p, rng, erng, closed, 0 if kind == "stochastic" else 4,
                     trees=case_roots(names, "reject3", "reject2"))


@pytest.mark.parametrize("row", ["uniform2", "uniform3", "uniform5", "uniform8", "uniform9", "zeros"])
@pytest.mark.parametrize("kind", ["stochastic", "sparse"])
def test_stochastic_uct_first_rollout_draw_on_every_threshold(ctx, monkeypatch, kind, row):
    from rl_agents_amd import native
    set_knobs(monkeypatch, "")
    rollout = ROWS[row]
    a = len(rollout)
    draws = cdf_draws(rollout)
    s0 = (np.arange(len(draws)) * 5 % S).astype(np.int32)
    erng = native.seed_sequence_states((), 77, len(draws))
    check_stochastic(ctx, stochastic_model(kind, S, a, zero_rewards=False), s0, 4, 5, np.ones(a) / a, rollout, cdf_records(draws), erng,
                     closed=(a % 2 == 0), records=0 if kind == "stochastic" else 4, trees=(0, len(draws) - 1))


@pytest.mark.parametrize("kind,width,knobs", [("stochastic", 0, ""), ("sparse", 2, ""), ("sparse", 2, "MP_UCT_STOCH_FUSED=2"),
                                               ("sparse", 3, ""), ("sparse", 4, ""), ("sparse", 5, ""),
                                               ("sparse", 3, "MP_UCT_STOCH_FUSED=0")])
def test_stochastic_uct_model_rows_on_every_threshold(ctx, monkeypatch, kind, width, knobs):
    """The ENV generator's record is forged: every episode's clone starts from it, so every episode's first model step draws on
    (or just below) a threshold of the root state's row -- fused records of 2 and 4 successors, 16- and 32-byte, rows of five
    by their thresholds, dense rows, and the unfused path."""
    from oracle import oracle
    from rl_agents_amd import native
    set_knobs(monkeypatch, knobs)
    a = 3
    records = {("stochastic", 0, ""): 0, ("sparse", 2, ""): 1, ("sparse", 2, "MP_UCT_STOCH_FUSED=2"): 2, ("sparse", 3, ""): 4,
               ("sparse", 4, ""): 4, ("sparse", 5, ""): 0, ("sparse", 3, "MP_UCT_STOCH_FUSED=0"): 0}[(kind, width, knobs)]
    cfg = stochastic_model(kind, S, a, zero_rewards=False, width=width)
    draws = []
    for s in range(S):
        draws += [(s, d) for d in cdf_draws(cfg["transition"][s, 0])]
    draws = draws[:64] if kind == "stochastic" else draws
    assert all((oracle.policy_cdf(cfg["transition"][s, j]) == oracle.policy_cdf(cfg["transition"][s, 0])).all()
               for s in range(S) for j in range(a))
    for lo in range(0, len(draws), 64):
        part = draws[lo:lo + 64]
        s0 = np.array([s for s, _ in part], dtype=np.int32)
        erng = cdf_records([d for _, d in part])
        rng = native.seed_sequence_states((), 55 + lo, len(part))
        p = np.ones(a) / a
        check_stochastic(ctx, cfg, s0, 4, 4, p, p, rng, erng, closed=True, records=records, trees=(0,))


# ---- mp_env_step_stochastic: one draw per call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", [("dense", 150), ("sparse", 1), ("sparse", 3), ("sparse", 4), ("sparse", 5)])
def test_env_step_stochastic_on_every_threshold(ctx, kind, width):
    """The expected next state is numpy.searchsorted(cdf, u, 'right') with cdf in numpy's own order."""
    import torch
    from oracle import oracle
    g = np.random.Generator(np.random.PCG64(width))
    n_states, a = (150, 2) if kind == "dense" else (20, 3)
    w = g.random((n_states, a, width)) + 0.05
    if width >= 3:
        w[:, :, 1::4] = 0.0                     # zero entries in the middle: repeated thresholds
    p = w / w.sum(axis=2, keepdims=True)
    reward = g.random((n_states, a))
    nxt = None
    if kind == "dense":
        model = ctx.load_dense(p, reward, None)
        rows = [(7, 1), (149, 0)]
    else:
        nxt = g.integers(0, n_states, size=(n_states, a, width)).astype(np.int64)
        model = ctx.load_sparse(p, nxt, reward, None)
        rows = [(s, s % a) for s in range(n_states)]
    cases = [(s, act, d) for s, act in rows for d in cdf_draws(p[s, act])]
    n = len(cases)
    erng = cdf_records([d for _, _, d in cases])
    want_state, want_rng = np.zeros(n, np.int32), erng.copy()
    for i, (s, act, (k53, _)) in enumerate(cases):
        cdf = oracle.policy_cdf(p[s, act])
        idx = int(np.searchsorted(cdf, k53 * 2.0 ** -53, side="right"))
        assert idx < width
        want_state[i] = idx if kind == "dense" else nxt[s, act, idx]
        st = forge.Stream(erng[i])
        assert st.random() == k53 * 2.0 ** -53
        want_rng[i] = st.record()
    dev = torch.device("cuda", ctx.device)
    d = dict(state=torch.tensor([s for s, _, _ in cases], dtype=torch.int32, device=dev), steps=torch.zeros(n, dtype=torch.int32, device=dev),
             alive=torch.ones(n, dtype=torch.uint8, device=dev),
             plans=torch.tensor([[act] for _, act, _ in cases], dtype=torch.int32, device=dev),
             gpow=torch.ones(4, dtype=torch.float64, device=dev), ret=torch.zeros(n, dtype=torch.float64, device=dev),
             disc=torch.zeros(n, dtype=torch.float64, device=dev), log=torch.full((n, 4), -1, dtype=torch.int32, device=dev),
             n_alive=torch.zeros(1, dtype=torch.int32, device=dev), erng=torch.from_numpy(erng.view(np.int64)).to(dev))
    torch.cuda.synchronize(dev)
    ctx.env_step_stochastic_device(model, d["state"], d["steps"], d["alive"], d["plans"], 4, d["gpow"], d["ret"], d["disc"], d["log"],
                                   d["n_alive"], d["erng"])
    ctx.synchronize()
    np.testing.assert_array_equal(d["state"].cpu().numpy(), want_state)
    np.testing.assert_array_equal(d["erng"].cpu().numpy().view(np.uint64), want_rng)
    assert np.array_equal(d["ret"].cpu().numpy(), np.array([reward[s, act] for s, act, _ in cases]))
    assert int(d["n_alive"].item()) == n and (d["steps"].cpu().numpy() == 1).all()
    model.close()


# ---- the optimistic planners: the plan's first choice --------------------------------------------------------------------------
def first_choice(rec, k):
    """The index, among the k tied actions, that numpy draws from the record (tests/test_forge_host.py holds forge.Stream to numpy)."""
    return forge.Stream(rec).below(k)


def masked_shape(k):
    return (8 if k < 8 else k), k


@pytest.mark.parametrize("variant,k", [(v, k) for v in ("lds", "ldsx", "global", "global_cls") for k in (3, 6, 7)] +
                         [("default", k) for k in (3, 70, 150)])     # (more actions than lanes: the plain kernel, no knob)
def test_opd_tie_draws(ctx, monkeypatch, variant, k):
    from oracle import oracle
    set_knobs(monkeypatch, "" if variant == "default" else "MP_OPD_MODEL=" + variant.split("_")[0] +
              (" MP_OPD_WIDE=cls" if variant.endswith("_cls") else ""))
    n_actions, k = masked_shape(k)
    t, r, term, avail = zero_table(S, n_actions, k)
    model = ctx.load_table(t, r, term, available=avail)
    rng, names = forge.tie_batch(k, N_TIE)
    rng0, rng_ref = rng.copy(), rng.copy()
    budget, s0 = 3 * n_actions, tie_roots()
    out = ctx.opd_plan(model, s0, budget, 0.8, 0.0, rng, max_plan_len=8)
    assert_form(ctx, "opd_any" if n_actions > 64 else {"lds": "opd_lds", "ldsx": "opd_ldsx", "global": "opd_wide_sib_small",
                                                        "global_cls": "opd_wide_cls_small", "default": "opd_lds"}[variant])
    ref = oracle.opd_plan_batch(t, r, term, s0, budget, 0.8, 0.0, rng_ref, max_plan_len=8, available=avail)
    for key in ("status", "plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    assert np.array_equal(out["root_lower"], ref["root_lower"]) and np.array_equal(out["root_upper"], ref["root_upper"])
    np.testing.assert_array_equal(rng, ref["rng_after"])
    assert out["plans"][:, 0].tolist() == [first_choice(rec, k) for rec in rng0]
    for root in case_roots(names, "reject3", "reject2"):
        tree = ctx.opd_tree(root, 1 + (budget // n_actions) * n_actions)
        one = oracle.opd_plan(t, r, term, int(s0[root]), budget, 0.8, 0.0, rng0[root].copy(), max_plan_len=8, available=avail)["tree"]
        for key in one:
            np.testing.assert_array_equal(tree[key], one[key], err_msg="tree[{}] of root {}".format(key, root))
    model.close()


@pytest.mark.parametrize("k", [3, 6, 7, 70, 150])
def test_opd_tie_draws_one_model_per_root(ctx, monkeypatch, k):
    from oracle import oracle
    set_knobs(monkeypatch, "")
    n_models = 5
    t, _, _, _ = zero_table(S, k, k)
    tr = np.stack([(t + m) % S for m in range(n_models)])
    rw, tm = np.zeros((n_models, S, k)), np.zeros((n_models, S), bool)
    model = ctx.load_table_batch(tr, rw, tm)
    mi = (np.arange(N_TIE) % n_models).astype(np.int32)
    rng, _ = forge.tie_batch(k, N_TIE)
    rng0, rng_ref = rng.copy(), rng.copy()
    out = ctx.opd_plan(model, tie_roots(), 3 * k, 0.8, 0.0, rng, max_plan_len=8, model_index=mi)
    assert_form(ctx, "opd_any" if k > 64 else "opd_lds")
    ref = oracle.opd_plan_each(tr, rw, tm, mi, tie_roots(), 3 * k, 0.8, 0.0, rng_ref, max_plan_len=8)
    for key in ("status", "plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    assert np.array_equal(out["root_lower"], ref["root_lower"]) and np.array_equal(out["root_upper"], ref["root_upper"])
    np.testing.assert_array_equal(rng, ref["rng_after"])
    assert out["plans"][:, 0].tolist() == [first_choice(rec, k) for rec in rng0]
    model.close()


@pytest.mark.parametrize("k", [3, 6, 7, 70, 150])
def test_robust_opd_tie_draws(ctx, monkeypatch, k):
    from oracle import oracle
    set_knobs(monkeypatch, "")
    n_actions, k = masked_shape(k)
    t, r, _, avail = zero_table(S, n_actions, k)
    tm, rm = np.stack([t, (t + 3) % S]), np.stack([r, r])
    av = np.stack([avail, avail])
    joint = ctx.load_joint(tm, rm, None, available=av)
    rng, names = forge.tie_batch(k, N_TIE)
    rng0, rng_ref = rng.copy(), rng.copy()
    budget, s0 = 3 * n_actions, tie_roots()
    out = ctx.ropd_plan(joint, s0, budget, 0.8, 0.0, rng, max_plan_len=8)
    assert_form(ctx, "ropd_any" if n_actions > 64 else "ropd_lds_m2")
    ref = oracle.ropd_plan_batch(tm, rm, None, np.repeat(s0[:, None], 2, axis=1), budget, 0.8, 0.0, rng_ref, max_plan_len=8, available=av)
    for key in ("status", "plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    assert np.array_equal(out["root_lower"], ref["root_lower"]) and np.array_equal(out["root_upper"], ref["root_upper"])
    np.testing.assert_array_equal(rng, ref["rng_after"])
    assert out["plans"][:, 0].tolist() == [first_choice(rec, k) for rec in rng0]
    for root in case_roots(names, "reject3"):
        tree = ctx.ropd_tree(root, 1 + (budget // n_actions) * n_actions, 2)
        one = oracle.ropd_plan(tm, rm, None, np.repeat(s0[root], 2), budget, 0.8, 0.0, rng0[root].copy(), max_plan_len=8,
                               available=av)["tree"]
        for key in one:
            np.testing.assert_array_equal(tree[key], one[key], err_msg="tree[{}] of root {}".format(key, root))
    joint.close()


SAOPD_MAPPINGS = {"wave": ("MP_SAOPD_MODEL=wave", "saopd_wave_lds", 3), "lane": ("MP_SAOPD_MODEL=lane", "saopd_lane", 3),
                  "wave-plain": ("MP_SAOPD_MODEL=wave MP_SAOPD_DICT=0 MP_SAOPD_LDS=0", "saopd_wave", 3),
                  "wave-dict": ("MP_SAOPD_MODEL=wave", "saopd_wave_dict", 13)}     # mapping -> knobs, form, expansions


@pytest.mark.parametrize("mapping,k", [(m, k) for m in ("wave", "lane") for k in (3, 6, 7, 70, 150)] +
                         [(m, k) for m in ("wave-plain", "wave-dict") for k in (3, 6, 7)])
def test_state_aware_opd_tie_draws(ctx, monkeypatch, mapping, k):
    """(get_plan runs twice per plan and the second descent is returned: the forged tie is the first one's, seen in the record
    after the plan and in everything the second descent draws.)  More than 64 actions plan on the lane kernel whatever the
    mapping asks for.  Three expansions need fewer depth entries than the LDS dictionaries are for, so "wave" keeps the whole
    arena of these 28 planners in LDS; "wave-dict" plans 13 expansions."""
    from oracle import oracle
    from rl_agents_amd import native
    knobs, form, expansions = SAOPD_MAPPINGS[mapping]
    set_knobs(monkeypatch, knobs)
    n_actions, k = masked_shape(k)
    t, r, term, avail = zero_table(S, n_actions, k)
    model = ctx.load_table(t, r, term, available=avail)
    planners = native.StateAwarePlanners(ctx, model, N_TIE)
    rng, _ = forge.tie_batch(k, N_TIE)
    rng0 = rng.copy()
    budget, s0 = expansions * n_actions, tie_roots()
    out = planners.plan(s0, budget, 0.8, 0.0, rng)
    # (zero rewards keep the backups going: 13 expansions of 6 or 7 tied actions fill the queue once, and the plan runs again)
    assert_form(ctx, "saopd_lane" if n_actions > 64 else form + ("_retry" if mapping == "wave-dict" and k in (6, 7) else ""))
    for i in range(N_TIE):
        o = oracle.saopd_plan(t, r, term, int(s0[i]), budget, 0.8, rng_state=rng0[i], max_plan_len=budget + 1, available=avail)
        assert out["status"][i] == 0, i
        np.testing.assert_array_equal(out["plans"][i, :out["plan_len"][i]], o["plan"], err_msg=str(i))
        assert out["env_steps"][i] == o["env_steps"] and out["updates"][i] == o["updates"], i
        np.testing.assert_array_equal(rng[i], o["rng_after"])
        if i % 7 in (3, 4):
            tree, sv = planners.export(i)
            assert np.array_equal(sv, o["state_values"]), i
            for key in ("parent", "first_child", "state", "depth", "lower", "reward", "alive", "count"):
                assert np.array_equal(tree[key], o["tree"][key]), (i, key)
    planners.close()
    model.close()


# ---- OLOP, BRUE, GBOP-D: against the restatements ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 6, 7, 70, 150])
def test_olop_tie_draws(monkeypatch, k):
    """The episode's seed draw takes one word; the uniform continuation among the k listed actions the forged ones (lead = 1)."""
    from rl_agents_amd.agents.common.factory import agent_factory
    from tests.test_gpu_olop import OLOP_AGENT, assert_tree, env_of, restated_root, BOUND_TOL
    set_knobs(monkeypatch, "")
    n_actions, k = masked_shape(k)
    t, r, term, avail = zero_table(S, n_actions, k)
    env = env_of(t, r, term, 0, avail if k < n_actions else None)
    cfg = {"gamma": 0.8, "episodes": 5, "horizon": 3, "upper_bound": {"type": "kullback-leibler"}, "continuation_type": "uniform"}
    agent = agent_factory(env, dict(cfg, __class__=OLOP_AGENT))
    planner = agent.planner
    rng, names = forge.tie_batch(k, N_TIE, lead=1)
    rng0, roots = rng.copy(), tie_roots()
    out = planner.plan_batch(env, roots, rng_states=rng)
    assert_form(planner.models.ctx, "olop_global")
    for i in range(N_TIE):
        res, rng_after = restated_root(t, r, term, roots[i], dict(planner.config), rng0[i], avail if k < n_actions else None)
        n = int(out["plan_len"][i])
        assert out["plans"][i, :n].tolist() == res["plan"].tolist(), i
        assert np.array_equal(rng[i], rng_after), i
        assert int(out["env_steps"][i]) == res["env_steps"], i
        assert abs(out["root_value"][i] - res["vu"][0]) <= BOUND_TOL, i
        if names[i] in ("reject2", "reject3"):
            tree = planner.models.ctx.olop_tree(i, 1 + 5 * 3 * n_actions)
            assert_tree(planner.relabel_tree(tree, planner._last_model), res, i)


@pytest.mark.parametrize("k", [3, 6, 7, 70, 150])
def test_brue_action_draws(monkeypatch, k):
    """A rollout's seed draw takes one word; its first integers(|A|) the forged ones (lead = 1)."""
    from rl_agents_amd.agents.common.factory import agent_factory
    from tests.test_gpu_brue import BRUE_AGENT, assert_tree, env_of, restated_root
    set_knobs(monkeypatch, "")
    t, r, term, _ = zero_table(S, k, k)
    tab = dict(mode="deterministic", transition=t, reward=r, terminal=term, next=None)
    env = env_of(tab, 0)
    agent = agent_factory(env, {"__class__": BRUE_AGENT, "budget": 24, "gamma": 0.9, "horizon": 4})
    planner = agent.planner
    rng, names = forge.tie_batch(k, N_TIE, lead=1)
    rng0, roots = rng.copy(), tie_roots()
    out = planner.plan_batch(env, roots, rng_states=rng)
    assert (out["status"] == 0).all()
    assert_form(planner.models.ctx, "brue_global")
    for i in range(N_TIE):
        res, rng_after = restated_root(tab, roots[i], planner.config, rng0[i])
        assert out["plans"][i].tolist() == res["plan"].tolist(), i
        assert np.array_equal(rng[i], rng_after), i
        assert int(out["env_steps"][i]) == res["env_steps"], i
        assert np.float64(out["root_value"][i]).view(np.uint64) == np.float64(res["root_value"]).view(np.uint64), i
        if names[i] in ("reject2", "reject3"):
            assert_tree(planner.models.ctx.brue_tree(i, planner._cap), res, i)


@pytest.mark.parametrize("k", [3, 6, 7, 70, 150])
def test_gbopd_tie_draws(ctx, monkeypatch, k):
    """The second run's sampling rule ties among the root's k listed actions: the plan's first draw."""
    from rl_agents_amd import native
    from tests import gbopd_restatement as gr
    set_knobs(monkeypatch, "")
    n_actions, k = masked_shape(k)
    t, r, term, avail = zero_table(S, n_actions, k)
    model = ctx.load_table(t, r, term, available=avail)
    planners = native.GraphBasedPlanners(ctx, model, N_TIE)
    rng, _ = forge.tie_batch(k, N_TIE)
    rng0, roots = rng.copy(), tie_roots()
    budget, gamma = 4 * n_actions, 0.9
    out = planners.plan(roots, budget, gamma, 1 / (1 - gamma), 1e-2, 5, rng)
    assert_form(ctx, "gbopd_wave_lds")
    assert (out["status"] == 0).all()
    for i in range(N_TIE):
        gen = generator_from(rng0[i])
        graph = gr.Graph(t, r, gamma, available=avail)
        plan = graph.plan(int(roots[i]), budget, 1e-2, 5, gen)
        assert out["plans"][i, :out["plan_len"][i]].tolist() == plan, i
        assert np.array_equal(rng[i], native.rng_state_from_generator(gen)), i
        assert gr.same_listing(planners.export(i), graph.listing()) == [], i
    planners.close()
    model.close()


# ---- MDP-GapE: against the restatement (tests/gape_cases.py builds the cases; tests/test_forge_host.py ties them to numpy) -------
def check_gape(case, names):
    from tests import gape_cases as gc
    from tests.test_gpu_gape import assert_tree
    from tests.test_gpu_gape_sweep import agent_of, assert_plan, device_tree
    env, agent = agent_of(case)
    planner, gamma = agent.planner, float(case["gamma"])
    rng = case["rng"].copy()
    out = planner.plan_batch(env, case["roots"], rng_states=rng)
    assert_form(planner.models.ctx, "gape_global")
    for i, (res, rng_after, seen) in enumerate(gc.restate_case(case)):
        assert res["error"] is None and gc.margin(seen) > gc.MARGIN, i
        assert_plan(out, i, res, rng_after, rng, gamma, i)           # plans, both arms, episodes run, env steps, record, root arms
        if names[i] in ("reject1", "reject2"):
            assert_tree(device_tree(planner.models.ctx, i, case["order"]), res, gamma, i)


@pytest.mark.parametrize("k,masked", [(k, False) for k in (3, 6, 7, 70, 150)] + [(70, True), (150, True)])
def test_gape_continuation_draws(monkeypatch, k, masked):
    """The episode's seed draw takes one word; integers(k) at the childless node below the root the forged ones (lead = 1)."""
    from tests import gape_cases as gc
    set_knobs(monkeypatch, "")
    check_gape(*gc.forged_continuation_case(k, masked))


@pytest.mark.parametrize("m", [3, 6, 7, 70, 150])
def test_gape_tie_draws(monkeypatch, m):
    """The first random_argmax among two or more: the m unvisited children of a node below the root, after three seed words."""
    from tests import gape_cases as gc
    set_knobs(monkeypatch, "")
    case, names, words = gc.forged_tie_case(m)
    assert words == 3
    check_gape(case, names)
