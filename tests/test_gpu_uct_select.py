"""mp_uct_step_tree_select: step_strategy "subtree" for a batch that shrinks and is re-ordered between two plans.  New root j
continues the subtree under child actions[j] of OLD root source_root[j], so a selection followed by a plan of the selected
roots must give, row for row, what re-rooting and planning the WHOLE batch gives for those roots -- on both layouts of
uct_kernel's trees and on the trees of the kernel that stores priors and child sets at expansion, with tables that change
between the two plans.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest

from tests.helpers import assert_form, assert_tree_equal, mdp_from_golden, uct_stoch_form

pytestmark = pytest.mark.gpu

S, EPISODES, HORIZON, GAMMA, TEMPERATURE = 12, 6, 3, 0.8, 10.0
OUT_KEYS = ("plans", "plan_len", "root_value", "root_child_count", "root_child_value", "env_steps")
# kind -> (|A|, tree layout of a fresh plan: A in 2..8 -> the 64-root interleaved layout 2, beyond -> root-major 0)
KINDS = {"a3": 3, "a9": 9, "stored": 3}


@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    yield c
    c.close()


def tables(n, a, seed0):
    from rl_agents_amd.envs import generators
    cfgs = [generators.random_deterministic(S, a, seed=seed0 + i, terminal_rate=0.2) for i in range(n)]
    return (np.stack([c["transition"] for c in cfgs]), np.stack([c["reward"] for c in cfgs]),
            np.stack([c["terminal"] for c in cfgs]).astype(np.uint8))


def policy_rows(a):
    """A listed policy over |A| = 3 with a per-state prior: every state lists two or three actions, priors differ by state."""
    rng = np.random.Generator(np.random.PCG64(77))
    listed = np.ones((S, a), dtype=bool)
    listed[np.arange(S), rng.integers(0, a, size=S)] = rng.random(S) < 0.5
    prior = np.where(listed, rng.random((S, a)) + 0.1, 0.0)
    prior = prior / prior.sum(axis=1, keepdims=True)
    return prior, listed


class Batch(object):
    """One batch model of n MDPs and the three ways this file plans on it."""

    def __init__(self, ctx, kind, n, seed0=10):
        self.ctx, self.kind, self.n, self.a = ctx, kind, n, KINDS[kind]
        self.t, self.r, self.term = tables(n, self.a, seed0)
        self.model = ctx.load_table_batch(self.t, self.r, self.term)
        self.policy = None
        self.p = np.ones(self.a) / self.a
        self.prior, self.listed = policy_rows(self.a) if kind == "stored" else (None, None)
        ctx.uct_reset_tree()

    def replace(self, which, seed0=500):
        """New tables for the MDPs `which` (policies are loaded again: they belong to the tables they were loaded for)."""
        t, r, term = tables(len(which), self.a, seed0)
        for k, i in enumerate(which):
            self.t[i], self.r[i], self.term[i] = t[k], r[k], term[k]
            self.model.update_tables(i, t[k:k + 1], r[k:k + 1], term[k:k + 1])
        if self.policy is not None:
            self.policy.close()
            self.policy = None

    def plan(self, index, states, rng, episodes=EPISODES, kept=False):
        """Plan, and assert the kernel form the plan recorded: `kept` = the plan continues trees armed by a step (whatever is
        left of them), else it starts fresh ones."""
        index, states = np.asarray(index, np.int32), np.asarray(states, np.int32)
        if self.kind == "stored":
            if self.policy is None:
                self.policy = self.ctx.load_policy(self.model, self.prior, self.prior, listed=self.listed)
            out = self.ctx.uct_plan_stochastic(self.model, index * S + states, episodes, HORIZON, GAMMA, TEMPERATURE, None, None, rng,
                                               closed_loop=False, max_plan_len=HORIZON, policy=self.policy)
        else:
            out = self.ctx.uct_plan(self.model, states, episodes, HORIZON, GAMMA, TEMPERATURE, self.p, self.p, rng,
                                    max_plan_len=HORIZON, model_index=index)
        assert_form(self.ctx, self.kept_form() if kept else self.fresh_form())
        return out

    def kept_form(self):
        return uct_stoch_form(0, 32, self.a, policy=True) if self.kind == "stored" else "uct_global"

    def fresh_form(self):
        """One MDP per root from fresh trees: a wavefront per root with its MDP in LDS where |A| has an unrolled form (2..8),
        else the global-memory kernel; the stored-prior kernel has one form for both."""
        return self.kept_form() if self.kind == "stored" else ("uct_lone_each" if self.a <= 8 else "uct_global")

    def tree(self, root):
        return self.ctx.uct_stoch_tree(root) if self.kind == "stored" else self.ctx.uct_tree(root)

    def next_states(self, states, actions):
        return self.t[np.arange(self.n), states, actions].astype(np.int32)

    def close(self):
        if self.policy is not None:
            self.policy.close()
        self.ctx.uct_reset_tree()
        self.model.close()


def first_plan(b):
    states = (np.arange(b.n) * 5 % S).astype(np.int32)
    from rl_agents_amd import native
    rng = native.seed_sequence_states((), 40, b.n)
    out = b.plan(np.arange(b.n), states, rng)
    first = np.where(out["plan_len"] > 0, out["plans"][:, 0], 0).astype(np.int32)
    return states, rng, out, first


def same_rows(out_b, rng_b, trees_b, out_a, rng_a, trees_a, rows):
    for k in OUT_KEYS:
        assert np.array_equal(out_b[k], out_a[k][rows]), k
    np.testing.assert_array_equal(rng_b, rng_a[rows])
    for tb, ta in zip(trees_b, trees_a):
        assert sorted(tb) == sorted(ta)
        for k in tb:
            assert np.array_equal(tb[k], ta[k]), "tree field " + k


def whole_batch(ctx, kind, n, changed, levels=1):
    """Run A: plan n roots, step every tree (`levels` times), replace the tables `changed`, plan all n again."""
    b = Batch(ctx, kind, n)
    states, rng, out, first = first_plan(b)
    second = np.where(out["plan_len"] > 1, out["plans"][:, 1], 0).astype(np.int32)
    ctx.uct_step_tree(first)
    nxt = b.next_states(states, first)
    if levels == 2:
        ctx.uct_step_tree(second)
        nxt = b.next_states(nxt, second)
    b.replace(changed)
    out2 = b.plan(np.arange(n), nxt, rng, kept=True)
    trees = [b.tree(i) for i in range(n)]
    b.close()
    return dict(out=out2, rng=rng, trees=trees)


@pytest.fixture(scope="module")
def run_a(ctx):
    """Run A per (kind, n, levels), planned once and shared."""
    memo = {}

    def get(kind, n, changed, levels=1):
        key = (kind, n, tuple(changed), levels)
        if key not in memo:
            memo[key] = whole_batch(ctx, kind, n, changed, levels)
        return memo[key]
    return get


# 70 -> 65: 64 distinct old roots in scrambled order (37 is coprime with 70) and old root 11 once more as NEW ROOT 64.  The new
# batch has two 64-root blocks like the old one: new roots 9, 11, 28, 45 and 62 of block 0 continue old roots 64, 68, 67, 66 and
# 65 of block 1, and new root 64 -- the one written into the second new block -- continues old root 11 of block 0, as new root 0 does.
SOURCES_65 = [(37 * j + 11) % 70 for j in range(64)] + [11]
assert len(set(SOURCES_65)) == 64 and SOURCES_65.count(11) == 2 and max(SOURCES_65) >= 64
CASES = [(6, [5, 2, 0], [2, 4]),
         (70, SOURCES_65, [11, 69])]


@pytest.mark.parametrize("n,sources,changed", CASES, ids=["6to3", "70to65"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_selection_equals_planning_the_whole_batch(ctx, run_a, kind, n, sources, changed):
    a = run_a(kind, n, changed)
    b = Batch(ctx, kind, n)
    states, rng, out, first = first_plan(b)
    src = np.asarray(sources, np.int32)
    ctx.uct_step_tree_select(src, first[src])
    nxt = b.next_states(states, first)
    b.replace(changed)
    rng_b = np.ascontiguousarray(rng[src])
    out2 = b.plan(src, nxt[src], rng_b, kept=True)
    trees = [b.tree(j) for j in range(len(src))]
    same_rows(out2, rng_b, trees, a["out"], a["rng"], [a["trees"][i] for i in sources], src)
    # the kept trees were continued, not started afresh: a continued root has more visits than one plan's episodes
    assert any(int(t["count"][0]) > EPISODES for t in trees)
    b.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_two_selections_before_one_plan_descend_two_levels(ctx, run_a, kind):
    n, first_sel, second_sel = 6, [5, 2, 0, 3], [2, 0, 3]          # (the second counts the roots of the first)
    a = run_a(kind, n, [2, 4], levels=2)
    b = Batch(ctx, kind, n)
    states, rng, out, first = first_plan(b)
    second = np.where(out["plan_len"] > 1, out["plans"][:, 1], 0).astype(np.int32)
    s1, s2 = np.asarray(first_sel, np.int32), np.asarray(second_sel, np.int32)
    rows = s1[s2]
    ctx.uct_step_tree_select(s1, first[s1])
    ctx.uct_step_tree_select(s2, second[rows])
    nxt = b.next_states(b.next_states(states, first), second)
    b.replace([2, 4])
    rng_b = np.ascontiguousarray(rng[rows])
    out2 = b.plan(rows, nxt[rows], rng_b, kept=True)
    trees = [b.tree(j) for j in range(len(rows))]
    same_rows(out2, rng_b, trees, a["out"], a["rng"], [a["trees"][i] for i in rows], rows)
    b.close()


def fresh_plan(ctx, kind, n, index, states, rng):
    b = Batch(ctx, kind, n)
    out = b.plan(index, states, rng)
    trees = [b.tree(j) for j in range(len(index))]
    b.close()
    return out, trees


@pytest.mark.parametrize("kind", list(KINDS))
def test_root_never_expanded_starts_a_fresh_tree(ctx, kind):
    from rl_agents_amd import native
    n, src = 6, np.asarray([4, 1], np.int32)
    b = Batch(ctx, kind, n)
    states = (np.arange(n) * 5 % S).astype(np.int32)
    rng = native.seed_sequence_states((), 40, n)
    b.plan(np.arange(n), states, rng, episodes=0)           # no episode: no root is expanded
    ctx.uct_step_tree_select(src, np.zeros(2, np.int32))
    rng_b, rng_f = np.ascontiguousarray(rng[src]), np.ascontiguousarray(rng[src])
    out = b.plan(src, states[src], rng_b, kept=True)
    trees = [b.tree(j) for j in range(2)]
    b.close()
    want, want_trees = fresh_plan(ctx, kind, n, src, states[src], rng_f)
    same_rows(out, rng_b, trees, want, rng_f, want_trees, np.arange(2))


def test_unlisted_action_starts_a_fresh_tree(ctx):
    n = 6
    b = Batch(ctx, "stored", n)
    states, rng, out, first = first_plan(b)
    unlisted = [(i, int(np.flatnonzero(~b.listed[states[i]])[0])) for i in range(n) if not b.listed[states[i]].all()]
    assert len(unlisted) >= 2, "the policy of this file lists fewer than |A| actions in some root states"
    src = np.asarray([i for i, _ in unlisted][::-1], np.int32)
    acts = np.asarray([a for _, a in unlisted][::-1], np.int32)
    ctx.uct_step_tree_select(src, acts)
    rng_b, rng_f = np.ascontiguousarray(rng[src]), np.ascontiguousarray(rng[src])
    nxt = states[src]                       # (any root state will do: both plans start from an empty root)
    got = b.plan(src, nxt, rng_b, kept=True)
    trees = [b.tree(j) for j in range(len(src))]
    b.close()
    want, want_trees = fresh_plan(ctx, "stored", n, src, nxt, rng_f)
    same_rows(got, rng_b, trees, want, rng_f, want_trees, np.arange(len(src)))


@pytest.mark.parametrize("kind", ["a3", "stored"])
def test_refused_selections_leave_the_trees_untouched(ctx, run_a, kind):
    from rl_agents_amd import native
    n = 6
    a = run_a(kind, n, [2, 4])
    b = Batch(ctx, kind, n)
    states, rng, out, first = first_plan(b)
    for source, actions in (([0, 6], [0, 0]), ([-1], [0]), ([], [])):      # outside the old batch; no root at all
        with pytest.raises(native.NativeError) as e:
            ctx.uct_step_tree_select(np.asarray(source, np.int32), np.asarray(actions, np.int32))
        assert e.value.code == native.MP_ERR_ARG
    ctx.uct_step_tree(first)
    nxt = b.next_states(states, first)
    b.replace([2, 4])
    out2 = b.plan(np.arange(n), nxt, rng, kept=True)
    same_rows(out2, rng, [b.tree(i) for i in range(n)], a["out"], a["rng"], a["trees"], np.arange(n))
    b.close()


@pytest.mark.parametrize("kind", ["a3", "stored"])
def test_device_arrays_grow_the_batch_and_start_afresh_outside_it(ctx, run_a, kind):
    """MP_MEM_DEVICE (torch tensors: the call only enqueues and cannot validate): a source outside the old batch starts a
    fresh tree instead of reading another one's; and a selection may name more roots than the old batch had."""
    import torch
    n, changed = 6, [2, 4]
    a = run_a(kind, n, changed)
    b = Batch(ctx, kind, n)
    states, rng, out, first = first_plan(b)
    sources = [5, 5, 2, 9, 0, 1, 3, -1]                  # 8 new roots from 6 old ones; 9 and -1 are no roots of the last plan
    rows = np.asarray([5, 5, 2, 1, 0, 1, 3, 4], np.int32)  # the MDP (and generator record) each new root plans on
    outside = [3, 7]
    src = torch.tensor(sources, dtype=torch.int32, device="cuda")
    act = torch.tensor(first[rows].tolist(), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.uct_step_tree_select(src, act)
    nxt = b.next_states(states, first)
    b.replace(changed)
    rng_b = np.ascontiguousarray(rng[rows])
    rng_f = np.ascontiguousarray(rng_b[outside])
    out2 = b.plan(rows, nxt[rows], rng_b, kept=True)
    trees = [b.tree(j) for j in range(len(rows))]
    kept = [j for j in range(len(rows)) if j not in outside]
    same_rows({k: out2[k][kept] for k in OUT_KEYS}, rng_b[kept], [trees[j] for j in kept], a["out"], a["rng"],
              [a["trees"][i] for i in rows[kept]], rows[kept])
    b.close()
    c = Batch(ctx, kind, n)
    c.replace(changed)
    want = c.plan(rows[outside], nxt[rows[outside]], rng_f)
    want_trees = [c.tree(j) for j in range(len(outside))]
    c.close()
    same_rows({k: out2[k][outside] for k in OUT_KEYS}, rng_b[outside], [trees[j] for j in outside], want, rng_f, want_trees,
              np.arange(len(outside)))


def test_device_tensors_of_another_type_are_refused(ctx):
    """An int64 tensor would be read as pairs of int32 values: the binding refuses it (and strided views) before the call."""
    import torch
    b = Batch(ctx, "a3", 6)
    first_plan(b)
    good = torch.zeros(2, dtype=torch.int32, device="cuda")
    for bad in (torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")[::2],
                torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32, device="cuda"), np.zeros(2, np.int32)):
        with pytest.raises(ValueError):
            ctx.uct_step_tree_select(bad, good)
        with pytest.raises(ValueError):
            ctx.uct_step_tree_select(good, bad)
    b.tree(5)               # (nothing was armed)
    b.close()


def test_closed_loop_trees_are_not_selected_from(ctx):
    from rl_agents_amd import native
    b = Batch(ctx, "a3", 6)
    rng = native.seed_sequence_states((), 40, 6)
    ctx.uct_plan_stochastic(b.model, np.arange(6, dtype=np.int32) * S, EPISODES, HORIZON, GAMMA, TEMPERATURE, b.p, b.p, rng,
                            closed_loop=True)
    assert_form(ctx, uct_stoch_form(0, 16, 3))
    with pytest.raises(native.NativeError) as e:
        ctx.uct_step_tree_select(np.asarray([1, 0], np.int32), np.zeros(2, np.int32))
    assert e.value.code == native.MP_ERR_ARG
    b.close()


def test_export_waits_for_the_plan_of_an_armed_selection(ctx):
    """Between a selection and its plan the workspaces hold the OLD batch: the exports refuse; dropping the selection
    (mp_uct_reset_tree) gives the last plan's trees back."""
    from rl_agents_amd import native
    b = Batch(ctx, "a3", 6)
    states, rng, out, first = first_plan(b)
    before = b.tree(5)
    ctx.uct_step_tree_select(np.asarray([5, 5, 5, 5, 5, 5, 5, 5], np.int32), np.zeros(8, np.int32))
    with pytest.raises(native.NativeError):
        b.tree(7)
    ctx.uct_reset_tree()
    after = b.tree(5)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    with pytest.raises(native.NativeError):
        b.tree(7)
    b.close()


@pytest.mark.parametrize("tag", ["subtree_large1", "subtree_highway"])
def test_plain_step_tree_still_replays_the_reference(ctx, golden, tag):
    """mp_uct_step_tree is the identity selection of the same kernels: tests/golden/uct.npz's kept-subtree episodes."""
    z = golden["uct"]
    p = "uct/" + tag
    cfg = mdp_from_golden(z, p + "/mdp")
    model = ctx.load_table(cfg["transition"], cfg["reward"], cfg["terminal"], max_steps=cfg["max_steps"])
    a = cfg["reward"].shape[1]
    rng = np.array(z[p + "/rng_before"], dtype=np.uint64).reshape(1, 6)
    prob = np.ones(a) / a
    ctx.uct_reset_tree()
    prev = None
    for step in range(int(z[p + "/n_steps"])):
        if prev is not None:
            ctx.uct_step_tree([prev])
        out = ctx.uct_plan(model, [int(z[p + "/states"][step])], int(z[p + "/episodes"]), int(z[p + "/horizon"]),
                           float(z[p + "/gamma"]), float(z[p + "/temperature"]), prob, prob, rng)
        q = "{}/step{}".format(p, step)
        np.testing.assert_array_equal(out["plans"][0, :int(out["plan_len"][0])], z[q + "/plan"], err_msg=q)
        np.testing.assert_array_equal(rng[0], z[q + "/rng_after"], err_msg=q)
        assert_tree_equal(z, q + "/tree", ctx.uct_tree(0), a, dict(count="count", value="value"))
        prev = int(out["plans"][0, 0])
    ctx.uct_reset_tree()
    model.close()


def test_plain_step_tree_still_replays_the_reference_on_stochastic_models():
    """... and tests/golden/stoch_subtree.npz's, the open-loop trees of the stochastic kernel (receding_horizon = 2 among
    them: two steps before one plan), through the replay the suite already has."""
    from tests.test_gpu_round3_goldens import test_mcts_subtree_strategy_on_stochastic_models_matches_reference as replay
    assert os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "stoch_subtree.npz"))
    replay()
