"""Forged draws for the planners that seed a model clone ON THE DEVICE, and for later draws of their plans: BRUE on dense and
sparse models, stochastic OLOP and Sparse Sampling (tests/test_gpu_forged_draws.py lists them as out of reach of a caller-passed
record; tests/forged_clone_cases.py builds the cases, tests/test_forge_host.py ties each of them to numpy on the host).

FORGE THE MODEL TO THE DRAW.  The clone's seed is ``x = next32() >> 2`` of the record the caller passes, its n-th random() is
numpy's own ``Generator(PCG64(SeedSequence(x))).random()`` = k53 * 2^-53, and the model row that draw meets is built from
integer weights n_j * 2^-53 that sum to 2^53 with n_0 + .. + n_b = k53: the draw sits ON cdf[b] (numpy answers b + 1, past every
zero entry behind it); the twin row has n_0 + .. + n_b = k53 + 1 and the same draw answers b.  A search written with `<` for
`<=` answers b for both twins (the host test checks that on numpy's 'left').  Seeds 0, 1 and 2^30 - 1 also put the device's
SeedSequence (seed_sequence.hpp) on the edges of its input.

  planner / form                               draw forged                                              rows
  BRUE brue_global, dense                      the clone's 1st draw (1st step of the 1st rollout);      W = 150: b = 0, 62, 63, 64, 127, 148
                                               its 2nd draw (2nd step, behind a one-hot row)            (a ballot full to its last lane, the
  BRUE brue_global, sparse B = 1, 3, 4, 5      the same                                                 `bal != ~0` exit); every b <= B - 2
  OLOP olop_stoch_dense / olop_stoch_sparse    the clone's 1st draw, continuation "zeros" (no word      the same
                                               before it) and "uniform" (one word)
  OLOP olop_stoch_dense, one-hot rows          forge.tie_batch(k, lead=1) on the uniform continuation   k = 3, 6, 7, 70, 150; a masked state
  Sparse Sampling ss_wave_lds / ss_wave_global the clone of ONE sample t* of the root: lanes 0, 1, 63   W = 2, 3, 150 dense and sparse;
      (MP_SS_FRAMES), horizon 1, |A| = 2,      of the first chunk, t* = 64 (first lane of the second    b = 0, W/2 - 1, W/2, W - 2
      C = 65; horizon 2 (the top level's C     chunk, action 0's last sample), 65 (action 1's first);
      samples on C lanes)                      seed words 0 and 0xFFFFFFFF; every record with and
                                               without a half buffered on entry
  Sparse Sampling root tie, mp_ss_plan and     the plan's LAST draw, after k * C sample words           k = 3, 6, 7, 70, 150 / 3, 6, 7
      mp_ss_plan_models (ss_each_lds / global) (forge.TIE_CASES but reject3: the samples take the
                                               buffered word)
  BRUE estimate(), through the planner         the 6th output: choice over counts (1, 1) at u = 0.5     one action, the chain of
                                               and one step below                                       forged_clone_cases.estimate_chain

Every comparison is on bits against the restatement driven by forge.Stream over the same record -- plan, exported tree, env_steps /
samples, root value, the generator record after the plan -- but OLOP's mu / value_upper / root value, within BOUND_TOL (the
device's log).

NOT HERE: estimate()'s choice over MORE than 64 outcomes (`le < m || base + m >= n`, brue_capture) on an exact cdf entry.  A plan
cannot be made to meet one; a device self-test of the choice as a function of its own was written and moved brue_kernel's
registers (profiles/brue_kernel_resources.txt), so it was left out."""
import numpy as np
import pytest

from rl_agents_amd import native
from rl_agents_amd.agents.tree_search.olop import OLOP
from tests import brue_restatement as brr
from tests import forge
from tests import forged_clone_cases as fc
from tests import olop_restatement as olr
from tests import olop_stoch_restatement as osr
from tests import sparse_sampling_restatement as ssr
from tests.helpers import assert_form
from tests.test_gpu_olop import BOUND_TOL
from tests.test_gpu_olop import assert_tree as assert_olop_tree

pytestmark = pytest.mark.gpu

N_ACTIONS = 3
BRUE = dict(budget=12, horizon=3, gamma=0.9)
OLOP_RUN = dict(episodes=4, horizon=3, gamma=0.8)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def load_model(ctx, cfg):
    if cfg["mode"] == "sparse":
        return ctx.load_sparse(cfg["transition"], cfg["next"], cfg["reward"], None)
    return ctx.load_dense(cfg["transition"], cfg["reward"], None)


# ---- BRUE ------------------------------------------------------------------------------------------------------------------------
def check_brue(ctx, cfg, roots, records, budget, horizon, gamma):
    model = load_model(ctx, cfg)
    rng = np.ascontiguousarray(records, dtype=np.uint64).copy()
    gp = np.asarray([gamma ** d for d in range(horizon + 1)], np.float64)
    out = ctx.brue_plan(model, roots, budget, horizon, gamma, gp, rng)
    assert_form(ctx, "brue_global")
    assert (out["status"] == 0).all()
    results = []
    for i, s0 in enumerate(roots):
        st = forge.Stream(records[i])
        res = brr.brue_plan(cfg["mode"], cfg["transition"], cfg["reward"], np.zeros(len(cfg["reward"]), bool), int(s0), budget, horizon,
                            gamma, st, nxt=cfg["next"])
        assert int(out["plans"][i]) == int(res["plan"][0]), i
        assert rng[i].tolist() == st.record(), i
        assert int(out["env_steps"][i]) == res["env_steps"], i
        assert bits(out["root_value"][i]) == bits(res["root_value"]), i
        tree = ctx.brue_tree(i, 1 + 2 * (budget + horizon))
        for k in brr.TREE_KEYS:
            assert np.array_equal(tree[k], res[k]), (i, k)
        assert np.array_equal(bits(tree["stat"]), bits(res["stat"])), (i, "stat bits")
        results.append(res)
    model.close()
    return results


@pytest.mark.parametrize("kind,W,step", [("stochastic", fc.DENSE_W, 0), ("stochastic", fc.DENSE_W, 1), ("sparse", 1, 0), ("sparse", 3, 0),
                                         ("sparse", 4, 0), ("sparse", 5, 0), ("sparse", 4, 1)])
def test_brue_clone_draw_on_and_below_every_threshold(ctx, kind, W, step):
    batch = fc.clone_twins(kind, W, N_ACTIONS, first="word", step=step)
    results = check_brue(ctx, batch["cfg"], batch["roots"], batch["records"], **BRUE)
    for c, res in zip(batch["cases"], results):       # (what the host test pins: the outcome node the forged row gives)
        if c["b"] is not None:
            want = c["want"] if kind == "stochastic" else int(batch["cfg"]["next"][c["state"], c["action"], c["want"]])
            assert res["key"][2 + 2 * step] == want


def test_brue_estimate_choice_on_the_boundary_through_the_planner(ctx):
    cfg = fc.estimate_chain()
    recs, ks = fc.estimate_records()
    results = check_brue(ctx, cfg, np.zeros(len(recs), np.int32), recs, fc.EST["budget"], fc.EST["horizon"], fc.EST["gamma"])
    for on, below in zip(results[0::2], results[1::2]):
        assert bits(on["stat"][1]) != bits(below["stat"][1])


# ---- stochastic OLOP -------------------------------------------------------------------------------------------------------------
def check_olop(ctx, cfg, roots, records, continuation, available=None, form=None, episodes=None, horizon=None, gamma=None, trees=None):
    model = load_model(ctx, cfg)
    if available is not None:
        model.set_available(available)
    model.set_episode_rules("source", 0)
    thr = olr.thresholds("4*np.log(time)", "global", episodes)
    rng = np.ascontiguousarray(records, dtype=np.uint64).copy()
    out = ctx.olop_plan_stochastic(model, roots, episodes, horizon, gamma, True, -1 if continuation == "uniform" else 0, thr,
                                   OLOP.value_upper_init(gamma, horizon), rng)
    assert_form(ctx, form)
    for i, s0 in enumerate(roots):
        st = forge.Stream(records[i])
        res = osr.olop_stoch_plan(cfg["mode"], cfg["transition"], cfg["reward"], None, int(s0), episodes, horizon, gamma, True, thr,
                                  continuation, st, next_states=cfg["next"], available=available)
        assert res["error"] is None and int(out["status"][i]) == native.MP_OK, i
        n = int(out["plan_len"][i])
        assert out["plans"][i, :n].tolist() == res["plan"].tolist(), i
        assert rng[i].tolist() == st.record(), i
        assert int(out["env_steps"][i]) == res["env_steps"], i
        assert abs(out["root_value"][i] - res["vu"][0]) <= BOUND_TOL, i
        if trees is None or i in trees:
            assert_olop_tree(ctx.olop_tree(i, 1 + episodes * horizon * cfg["reward"].shape[1]), res, i)
    model.close()


@pytest.mark.parametrize("continuation", ["zeros", "uniform"])
@pytest.mark.parametrize("kind,W", [("stochastic", fc.DENSE_W), ("sparse", 3), ("sparse", 4), ("sparse", 5)])
def test_olop_stoch_clone_draw_on_and_below_every_threshold(ctx, kind, W, continuation):
    batch = fc.clone_twins(kind, W, N_ACTIONS, first="word" if continuation == "uniform" else "zeros")
    check_olop(ctx, batch["cfg"], batch["roots"], batch["records"], continuation,
               form="olop_stoch_dense" if kind == "stochastic" else "olop_stoch_sparse", **OLOP_RUN)


@pytest.mark.parametrize("k", fc.TIE_KS)
def test_olop_stoch_uniform_continuation_tie_draws(ctx, k):
    """olop_stoch_kernel's own gen.below(k): seed word, then the forged words (lead = 1), k < |A| listed in a masked state."""
    from tests.test_gpu_forged_draws import N_TIE, tie_roots
    n_actions = 8 if k < 8 else k
    cfg, _, avail = fc.one_hot_tie_model(12, n_actions, k)
    rng, names = forge.tie_batch(k, N_TIE, lead=1)
    check_olop(ctx, cfg, tie_roots(), rng, "uniform", available=avail, form="olop_stoch_dense",
               trees=[i for i, c in enumerate(names) if c in ("reject2", "reject1")][:4], **OLOP_RUN)


# ---- Sparse Sampling -------------------------------------------------------------------------------------------------------------
def check_ss(ctx, model, tab, roots, records, horizon, C, gamma, form, available=None, model_index=None):
    rng = np.ascontiguousarray(records, dtype=np.uint64).copy()
    out = ctx.ss_plan(model, roots, horizon, C, gamma, rng, model_index=model_index)
    assert_form(ctx, form)
    assert (out["status"] == 0).all()
    results = []
    for i, s0 in enumerate(roots):
        st = forge.LoggingStream(records[i])
        res = ssr.ss_plan(tab["mode"], tab["transition"], tab["reward"], int(s0), horizon, C, gamma, st, nxt=tab.get("next"),
                          available=available)
        assert int(out["plans"][i]) == int(res["plan"][0]), i
        assert rng[i].tolist() == st.record(), i
        assert int(out["samples"][i]) == res["samples"], i
        assert bits(out["root_value"][i]) == bits(res["root_value"]), i
        tree = ctx.ss_tree(i)
        for k in ssr.TREE_KEYS:
            assert np.array_equal(tree[k], res[k]), (i, k)
        assert np.array_equal(bits(tree["value"]), bits(res["value"])), (i, "value bits")
        results.append((res, st))
    return results


@pytest.mark.parametrize("frames,form", [("lds", "ss_wave_lds"), ("global", "ss_wave_global")])
@pytest.mark.parametrize("kind,W,horizon", [("stochastic", 150, 1), ("sparse", 2, 1), ("sparse", 3, 1), ("stochastic", 2, 1),
                                            ("stochastic", 3, 1), ("sparse", 3, 2)])
def test_sparse_sampling_one_samples_clone_on_and_below_every_threshold(ctx, monkeypatch, kind, W, horizon, frames, form):
    monkeypatch.setenv("MP_SS_FRAMES", frames)
    for batch in fc.ss_batches(kind, W, horizon):
        model = load_model(ctx, batch["cfg"])
        check_ss(ctx, model, batch["cfg"], batch["roots"], batch["records"], horizon, fc.SS_C, 0.9, form)
        model.close()


def ss_tie_setup(k):
    from tests.helpers import zero_table
    n_actions = 8 if k < 8 else k
    t, r, term, avail = zero_table(12, n_actions, k)
    n = 2 * len(fc.SS_TIE_CASES)
    recs, names, expect = fc.ss_tie_batch(k, n, k * fc.SS_TIE_C)
    roots = (np.arange(n) * 5 % 12).astype(np.int32)
    return (t, r, term), (avail if k < n_actions else None), recs, expect, roots


def assert_ties_met(results, k, expect):
    for (res, st), e in zip(results, expect):
        assert st.log[-1][0] == "below" and st.log[-1][1] == k * fc.SS_TIE_C and st.log[-1][3] == k
        assert e is None or st.log[-1][4] == e


@pytest.mark.parametrize("k", fc.TIE_KS)
def test_sparse_sampling_root_tie_draws(ctx, monkeypatch, k):
    monkeypatch.delenv("MP_SS_FRAMES", raising=False)
    (t, r, term), avail, recs, expect, roots = ss_tie_setup(k)
    model = ctx.load_table(t, r, term, available=avail)
    tab = dict(mode="deterministic", transition=t, reward=r)
    assert_ties_met(check_ss(ctx, model, tab, roots, recs, 1, fc.SS_TIE_C, 0.9, "ss_wave_lds", available=avail), k, expect)
    model.close()


@pytest.mark.parametrize("each", ["lds", "global"])
@pytest.mark.parametrize("k", [3, 6, 7])
def test_sparse_sampling_root_tie_draws_one_model_per_root(ctx, monkeypatch, k, each):
    """Five copies of the table as a batch model: root i plans on copy i % 5 from its LOCAL state; the exported keys of decision
    nodes are GLOBAL states."""
    monkeypatch.setenv("MP_EACH_MODEL", each)
    (t, r, term), avail, recs, expect, roots = ss_tie_setup(k)
    n_models, S = 5, t.shape[0]
    model = ctx.load_table_batch(np.stack([t] * n_models), np.stack([r] * n_models), np.stack([term] * n_models))
    if avail is not None:
        model.set_available(np.concatenate([avail] * n_models))
    mi = (np.arange(len(roots)) % n_models).astype(np.int32)
    rng = recs.copy()
    out = ctx.ss_plan(model, roots, 1, fc.SS_TIE_C, 0.9, rng, model_index=mi)
    assert_form(ctx, "ss_each_" + each)
    assert (out["status"] == 0).all()
    for i, s0 in enumerate(roots):
        st = forge.LoggingStream(recs[i])
        res = ssr.ss_plan("deterministic", t, r, int(s0), 1, fc.SS_TIE_C, 0.9, st, available=avail)
        assert st.log[-1][1] == k * fc.SS_TIE_C and st.log[-1][3] == k and (expect[i] is None or st.log[-1][4] == expect[i])
        assert int(out["plans"][i]) == int(res["plan"][0]), i
        assert rng[i].tolist() == st.record(), i
        assert int(out["samples"][i]) == res["samples"] and bits(out["root_value"][i]) == bits(res["root_value"]), i
        tree = ctx.ss_tree(i)
        decision = (np.asarray(res["is_chance"]) == 0) & (np.asarray(res["parent"]) >= 0)
        assert np.array_equal(tree["key"], np.where(decision, res["key"] + int(mi[i]) * S, res["key"])), i
        for key in ("parent", "is_chance", "depth", "count"):
            assert np.array_equal(tree[key], res[key]), (i, key)
        assert np.array_equal(bits(tree["value"]), bits(res["value"])), i
    model.close()
