"""Shared helpers for the parity tests."""
import numpy as np


def mdp_from_golden(z, prefix):
    """Rebuild the finite-MDP config stored by make_golden.put_mdp."""
    cfg = dict(mode=str(z[prefix + "/mode"]), transition=z[prefix + "/transition"], reward=z[prefix + "/reward"],
               terminal=z[prefix + "/terminal"], max_steps=int(z[prefix + "/max_steps"]))
    if cfg["mode"] == "sparse":
        cfg["next"] = z[prefix + "/next"]
    return cfg


def bfs_order(parent, first_child, n_actions):
    """Creation-order tree arrays -> canonical BFS permutation (same order make_golden.bfs_tree uses).

    Returns (order, bfs_parent, bfs_action): order[i] = creation index of the i-th BFS node.
    """
    order, bpar, bact = [0], [-1], [-1]
    i = 0
    while i < len(order):
        fc = int(first_child[order[i]])
        if fc >= 0:
            for a in range(n_actions):
                order.append(fc + a)
                bpar.append(i)
                bact.append(a)
        i += 1
    return np.asarray(order), np.asarray(bpar, np.int32), np.asarray(bact, np.int32)


def assert_tree_equal(z, prefix, tree, n_actions, fields):
    """Compare a creation-order tree (dict of arrays) with a golden BFS tree, bit for bit."""
    order, bpar, bact = bfs_order(tree["parent"], tree["first_child"], n_actions)
    assert len(order) == len(z[prefix + "/parent"]), (len(order), len(z[prefix + "/parent"]))
    np.testing.assert_array_equal(bpar, z[prefix + "/parent"])
    np.testing.assert_array_equal(bact, z[prefix + "/action"])
    for gold_name, mine in fields.items():
        got = np.asarray(tree[mine])[order]
        want = z[prefix + "/" + gold_name]
        assert np.array_equal(got.astype(want.dtype), want), "tree field {} differs".format(gold_name)


def replay_state_aware_episode(z, name, plan_fn):
    """Replay one golden StateAwarePlannerAgent episode (consecutive plan() calls on one planner) and compare every
    plan, tree, leaves set, state-value table, env-step count and generator state with the reference's.

    plan_fn(cfg, s0, params, rng, planner_state) -> dict(plan, env_steps, rng_after, tree, state_values, planner);
    raises ValueError where the reference does.  tree: creation-order arrays re-based at the root."""
    import pytest
    p = "sa/" + name
    cfg = mdp_from_golden(z, p + "/mdp")
    a = cfg["reward"].shape[1]
    params = dict(budget=int(z[p + "/budget"]), gamma=float(z[p + "/gamma"]),
                  terminal_reward=float(z[p + "/terminal_reward"]), accuracy=float(z[p + "/accuracy"]),
                  backup_aggregated_nodes=bool(z[p + "/backup_aggregated_nodes"]),
                  prune_suboptimal_leaves=bool(z[p + "/prune_suboptimal_leaves"]))
    rng = np.array(z[p + "/rng_before"], dtype=np.uint64)
    raises_at = int(z[p + "/raises_at_step"]) if p + "/raises_at_step" in z.files else -1
    planner, env_steps = None, 0
    for step in range(int(z[p + "/n_steps"])):
        s0 = int(z[p + "/states"][step])
        if step == raises_at:
            with pytest.raises(ValueError):
                plan_fn(cfg, s0, params, rng, planner)
            break
        out = plan_fn(cfg, s0, params, rng, planner)
        q = "{}/step{}".format(p, step)
        np.testing.assert_array_equal(out["plan"], z[q + "/plan"], err_msg=q)
        np.testing.assert_array_equal(out["rng_after"], z[q + "/rng_after"], err_msg=q)
        env_steps += int(out["env_steps"])
        assert env_steps == int(z[q + "/env_steps"]), q
        tree = out["tree"]
        assert int(tree["alive"].sum()) == int(z[q + "/n_leaves"]), q
        assert_tree_equal(z, q + "/tree", tree, a, dict(count="count", lower="lower", reward="reward", done="done",
                                                        depth="depth", obs="state", is_leaf="alive"))
        want = z[q + "/state_values"]
        seen = ~np.isnan(want)              # states the reference's defaultdict holds; the others are at the default
        assert np.array_equal(out["state_values"][seen], want[seen]), q
        assert np.all(out["state_values"][~seen] == 1 / (1 - params["gamma"])), q
        planner, rng = out["planner"], out["rng_after"]


def bfs_children(first_child, n_children):
    """Creation-order trees whose nodes have a variable number of (contiguous) children -> BFS permutation and the BFS
    parent index of every node (the order make_golden_variants.keyed_tree lists a reference tree in)."""
    order, bpar = [0], [-1]
    i = 0
    while i < len(order):
        n = order[i]
        for j in range(int(n_children[n])):
            order.append(int(first_child[n]) + j)
            bpar.append(i)
        i += 1
    return np.asarray(order), np.asarray(bpar, np.int32)


def assert_keyed_tree_equal(z, prefix, tree, fields):
    """Compare a creation-order tree with per-node `action` keys and `n_children` with a golden keyed BFS tree."""
    order, bpar = bfs_children(tree["first_child"], tree["n_children"])
    assert len(order) == len(z[prefix + "/parent"]), (len(order), len(z[prefix + "/parent"]))
    np.testing.assert_array_equal(bpar, z[prefix + "/parent"])
    np.testing.assert_array_equal(np.asarray(tree["action"])[order], z[prefix + "/action"])
    for gold_name, mine in fields.items():
        got = np.asarray(tree[mine])[order]
        want = z[prefix + "/" + gold_name]
        assert np.array_equal(got.astype(want.dtype), want), "tree field {} differs".format(gold_name)


def reference_policy_lists(policy_config, available, order=None):
    """What the reference's policy functions return, state by state, on an environment whose
    get_available_actions() lists flatnonzero(available[s]) (mcts.py:46-97) -- or, with ``order`` (a permutation of the
    action ids), lists the available actions in that order: dict(actions=[...], p=[...]).
    Restated here for the tests only (the oracle consumes the lists; the product builds [S, A] tables of its own)."""
    available = np.asarray(available).astype(bool)
    n_states, n_actions = available.shape
    actions, probs = [], []
    for s in range(n_states):
        av = np.flatnonzero(available[s]) if order is None else np.asarray([a for a in order if available[s, a]])
        kind = policy_config["type"]
        if kind == "random":                                  # mcts.py:46-57: ignores availability
            a, p = np.arange(n_actions), np.ones(n_actions) / n_actions
        elif kind == "random_available":                      # mcts.py:59-73
            a, p = av, np.ones(len(av)) / len(av)
        elif kind == "preference":                            # mcts.py:75-97
            a, p = av, np.ones(len(av)) / len(av)
            for i in range(len(av)):
                if av[i] == policy_config["action"]:
                    p = np.ones(len(av)) / (len(av) - 1 + policy_config["ratio"])
                    p[i] *= policy_config["ratio"]
                    break
        else:
            raise ValueError("Unknown policy type")
        actions.append([int(x) for x in a])
        probs.append(np.asarray(p, dtype=np.float64))
    return dict(actions=actions, p=probs)


def restricted_agent_policy_lists(table, available, order=None):
    """MCTSWithPriorPolicyAgent.agent_policy_available (mcts_with_prior.py:56-62): the prior agent's distribution
    restricted to the available actions (in the env's listing order) and renormalised with numpy's sum."""
    available = np.asarray(available).astype(bool)
    actions, probs = [], []
    for s in range(available.shape[0]):
        av = np.flatnonzero(available[s]) if order is None else np.asarray([a for a in order if available[s, a]])
        p = np.array([table[s, a] for a in av])
        p /= np.sum(p)
        actions.append([int(x) for x in av])
        probs.append(p)
    return dict(actions=actions, p=probs)


def bfs_by_parent(parent):
    """Creation-order parent array -> BFS permutation in which a node's children come in ascending id = the order in
    which the reference inserted them into its `children` dict (expansion order for action nodes, first-visit order for
    observation nodes).  -> (order, bfs_parent)."""
    kids = [[] for _ in parent]
    for i, p in enumerate(parent):
        if p >= 0:
            kids[int(p)].append(i)
    order, bpar = [0], [-1]
    i = 0
    while i < len(order):
        for c in kids[order[i]]:
            order.append(c)
            bpar.append(i)
        i += 1
    return np.asarray(order), np.asarray(bpar, np.int32)


def assert_parent_tree_equal(z, prefix, tree, fields):
    """Compare a creation-order tree given by `parent` / `action` (= key) arrays with a golden keyed BFS tree."""
    order, bpar = bfs_by_parent(tree["parent"])
    assert len(order) == len(z[prefix + "/parent"]), (len(order), len(z[prefix + "/parent"]))
    np.testing.assert_array_equal(bpar, z[prefix + "/parent"])
    np.testing.assert_array_equal(np.asarray(tree["action"])[order], z[prefix + "/action"])
    for gold_name, mine in fields.items():
        got = np.asarray(tree[mine])[order]
        want = z[prefix + "/" + gold_name]
        assert np.array_equal(got.astype(want.dtype), want), "tree field {} differs".format(gold_name)


def replay_state_aware_masked_episode(z, name, plan_fn):
    """Replay one golden StateAwarePlannerAgent episode on an environment that restricts its actions
    (tests/golden/round3.npz, sa_masked/*): every plan, keyed tree, leaves set, state-value table, env-step count and
    generator state.  plan_fn(cfg, available, order, s0, params, rng, planner_state) -> dict(plan, env_steps, rng_after,
    tree, state_values, planner) in the ENVIRONMENT's action ids; `order` = the env's listing order (None = ascending);
    tree: creation-order arrays re-based at the root with `action`, `n_children`, `alive`.  Raises where the reference does."""
    import pytest
    p = "sa_masked/" + name
    cfg = mdp_from_golden(z, p + "/mdp")
    params = dict(budget=int(z[p + "/budget"]), gamma=float(z[p + "/gamma"]),
                  terminal_reward=float(z[p + "/terminal_reward"]), accuracy=float(z[p + "/accuracy"]),
                  backup_aggregated_nodes=bool(z[p + "/backup_aggregated_nodes"]),
                  prune_suboptimal_leaves=bool(z[p + "/prune_suboptimal_leaves"]))
    order = [1, 0, 2, 3, 4] if bool(z[p + "/listing_idle_first"]) else None
    rng = np.array(z[p + "/rng_before"], dtype=np.uint64)
    raises_at = int(z[p + "/raises_at_step"]) if p + "/raises_at_step" in z.files else -1
    planner, env_steps = None, 0
    n_steps = int(z[p + "/n_steps"])
    for step in range(n_steps):
        s0 = int(z[p + "/states"][step])
        if step == raises_at:
            with pytest.raises(ValueError):
                plan_fn(cfg, z[p + "/available"], order, s0, params, rng, planner)
            break
        out = plan_fn(cfg, z[p + "/available"], order, s0, params, rng, planner)
        q = "{}/step{}".format(p, step)
        np.testing.assert_array_equal(out["plan"], z[q + "/plan"], err_msg=q)
        np.testing.assert_array_equal(out["rng_after"], z[q + "/rng_after"], err_msg=q)
        env_steps += int(out["env_steps"])
        assert env_steps == int(z[q + "/env_steps"]), q
        tree = out["tree"]
        assert int(np.asarray(tree["alive"]).sum()) == int(z[q + "/n_leaves"]), q
        assert_keyed_tree_equal(z, q + "/tree", tree, dict(count="count", lower="lower", reward="reward", done="done",
                                                          depth="depth", obs="state", is_leaf="alive"))
        want = z[q + "/state_values"]
        seen = ~np.isnan(want)
        assert np.array_equal(out["state_values"][seen], want[seen]), q
        assert np.all(out["state_values"][~seen] == 1 / (1 - params["gamma"])), q
        planner, rng = out["planner"], out["rng_after"]
    assert raises_at >= 0 or n_steps > 0


def first_result(queue, procs, seconds):
    """The first item the ranks put on `queue` -- or a test failure, not a hang, when a rank dies or nothing arrives within
    `seconds` (a crashed rank leaves the others blocked in a collective forever; every process is killed then)."""
    import time
    import pytest
    deadline = time.time() + seconds
    while time.time() < deadline:
        if not queue.empty():
            return queue.get()
        if any(p.exitcode not in (None, 0) for p in procs):
            break
        time.sleep(0.02)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    pytest.fail("the process group produced no result (exit codes {}; still running ones were killed)".format(codes))


# ---- shared by the forged-draw tests (tests/test_forge_host.py, tests/test_gpu_forged_draws.py) and tests/test_host_logic.py
M64 = (1 << 64) - 1


def scalar_mulhi(a, b):
    a0, a1, b0, b1 = a & 0xffffffff, a >> 32, b & 0xffffffff, b >> 32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> 32) + (p01 & 0xffffffff) + (p10 & 0xffffffff)
    return (p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32)) & M64


def scalar_step(s_hi, s_lo, inc_hi, inc_lo):
    """Pcg64U::advance of csrc/pcg64.hpp on Python integers masked to 64 bits (tests/test_host_logic.py checks it against numpy,
    tests/test_forge_host.py steps it on forged records)."""
    m_lo, m_hi = 0x4385DF649FCCF645, 0x2360ED051FC65DA4
    lo = (s_lo * m_lo) & M64
    hi = (scalar_mulhi(s_lo, m_lo) + s_lo * m_hi + s_hi * m_lo) & M64
    lo2 = (lo + inc_lo) & M64
    carry = ((lo & inc_lo) | ((lo | inc_lo) & (~lo2 & M64))) >> 63
    return (hi + inc_hi + carry) & M64, lo2


def scalar_output(s_hi, s_lo):
    x, rot = s_hi ^ s_lo, s_hi >> 58
    return ((x >> rot) | (x << ((64 - rot) & 63))) & M64


def generator_from(rec):
    """A numpy Generator(PCG64) standing at the six-word record ``rec``."""
    from rl_agents_amd import native
    gen = np.random.Generator(np.random.PCG64(0))
    native.generator_set_state(gen, rec)
    return gen


def zero_table(n_states, n_actions, k):
    """All rewards zero, no terminal state, no self-loop: every first decision is a tie among the ``k`` listed actions."""
    t = (np.arange(n_states)[:, None] + 1 + np.arange(n_actions)[None, :] % (n_states - 1)) % n_states
    avail = np.zeros((n_states, n_actions), bool)
    avail[:, :k] = True
    return t.astype(np.int64), np.zeros((n_states, n_actions)), np.zeros(n_states, bool), avail


def value_table(n_states, n_actions):
    """No terminal state; rewards on a grid of 17 values, different for every action of a state: the first rollout action shows
    in every statistic."""
    s, a = np.arange(n_states)[:, None], np.arange(n_actions)[None, :]
    return ((s * 5 + a * 3 + 1) % n_states).astype(np.int64), ((s * 7 + a * 11) % 17) / 16.0, np.zeros(n_states, bool)


def stochastic_model(kind, n_states, n_actions, zero_rewards, width=3):
    """A dense ("stochastic") or sparse model whose rows depend on the state alone (every action of a state samples the same
    row, with a zero entry in it), so that the env generator's first draw meets the row of the root state whatever the first
    action is.  No terminal state."""
    g = np.random.Generator(np.random.PCG64(100 + n_actions + width))
    reward = np.zeros((n_states, n_actions)) if zero_rewards else value_table(n_states, n_actions)[1]
    if kind == "sparse":
        w = g.random((n_states, 1, width)) + 0.05
        if width >= 3:
            w[:, :, 1] = 0.0
        p = np.repeat(w / w.sum(axis=2, keepdims=True), n_actions, axis=1)
        nxt = g.integers(0, n_states, size=(n_states, n_actions, width)).astype(np.int64)
        return dict(mode="sparse", transition=p, next=nxt, reward=reward)
    w = g.random((n_states, 1, n_states)) + 0.05
    w[:, :, 2::3] = 0.0
    p = np.repeat(w / w.sum(axis=2, keepdims=True), n_actions, axis=1)
    return dict(mode="stochastic", transition=p, next=None, reward=reward)


# rows whose inverse-CDF thresholds the forged-draw tests meet exactly
CDF_ROWS = {
    "uniform2": np.ones(2) / 2, "uniform3": np.ones(3) / 3, "uniform5": np.ones(5) / 5, "uniform8": np.ones(8) / 8,
    "uniform9": np.ones(9) / 9,
    "zeros": np.array([0.25, 0.0, 0.5, 0.25, 0.0, 0.0]),          # a zero in the middle (a repeated threshold), trailing zeros
    "lead_zero": np.array([0.0, 0.3, 0.0, 0.7]),                  # a threshold of 0: no k is below it
}


# ---- kernel forms (Context.last_kernel_variant()): what a test means to run, asserted after the call.  opd_form and saopd_form
# restate the host's choice (csrc/opd_host.hpp opd_shape, csrc/saopd.hip mp_saopd_plan) from the shape of a call and the knobs
# the test set, so that a test says "the knob I set took effect" without hard-coding a name per shape.
LDS_AVAIL = 160 * 1024 - 1024


def assert_form(ctx, name):
    """The last plan / batched VI call on ``ctx`` launched the kernel form ``name``."""
    got = ctx.last_kernel_variant()
    assert got == name, "kernel form {!r} ran where the test means {!r}".format(got, name)


def assert_vi_batch_form(ctx, N, S, A, iters):
    """The last vi_solve_batch on ``ctx`` -- N MDPs of S states and A actions -- launched the form the host query names for it
    (native.vi_batch_geometry: the function the solve launches from, with the knobs as the test has set them)."""
    from rl_agents_amd import native
    assert_form(ctx, native.vi_batch_geometry(N, S, A, iters, cus=ctx.device_info()["n_cu"])["name"])


def opd_closing_fits(n_actions, budget):
    """closing_compact_fits (csrc/opd_closing.hpp) at the sizes opd_shape derives from |A| and the budget."""
    k = budget // n_actions
    cap = 1 + k * n_actions
    t = ((cap + 63) // 64) | 1
    return n_actions <= 255 and k < (1 << 22) and 16 * k + 4 * cap <= 64 * t * 8


def opd_form(ctx, n_actions, budget, n_roots, model=None, wide=None, closing=None, general=False, models=0):
    """The form mp_opd_plan (``models`` = 0) or mp_ropd_plan (``models`` = M) records: ``model`` / ``wide`` / ``closing`` are the
    values of MP_OPD_MODEL / MP_OPD_WIDE / MP_OPD_CLOSING (None: unset), ``general``: MP_OPD_LOOP=0, a negative terminal reward
    or gamma outside [0, 1)."""
    prefix = "ropd" if models else "opd"
    if n_actions > 64:
        return prefix + "_any"
    cus = ctx.device_info()["n_cu"]
    k = budget // n_actions
    cap = 1 + k * n_actions
    t = ((cap + 63) // 64) | 1
    lds_bounds = 64 * t * 8
    lds_full = lds_bounds + max(k, 1) * 4
    glb = lds_bounds > LDS_AVAIL or n_roots > cus * (LDS_AVAIL // lds_bounds)
    if model == "global":
        glb = True
    if model in ("lds", "ldsx") and lds_bounds <= LDS_AVAIL:
        glb = False
    if glb:
        sib = wide != "cls"
        small = (((k + 64) // 64) * n_actions if sib else t) <= 128
        return "{}_wide_{}{}{}".format(prefix, "sib" if sib else "cls", "_small" if small and not models else "",
                                       "_gen" if general else "")
    expg = lds_full > LDS_AVAIL or n_roots > cus * (LDS_AVAIL // lds_full) or model == "ldsx"
    chain = closing == "chain" or not opd_closing_fits(n_actions, budget)
    if models:
        loop = "_gen" if general or models > 4 else "_m2" if models <= 2 else "_m4"
    else:
        loop = "_gen" if general else ""
    return "{}_{}{}{}".format(prefix, "ldsx" if expg else "lds", loop, "_chain" if chain else "")


def saopd_form(ctx, n_states, n_actions, budget, n_planners, nodes_before=0, model=None, lds=None, dictionary=None, order=None,
               have_cost=False, queue=None, retry=False, device_arrays=False):
    """The form mp_saopd_plan records for one plan of a planner batch that holds ``nodes_before`` nodes per planner: ``model`` /
    ``lds`` / ``dictionary`` / ``order`` / ``queue`` are the values of MP_SAOPD_MODEL / _LDS / _DICT / _ORDER / _QUEUE (None:
    unset); ``have_cost``: the planners have planned before, or -- fresh ones -- an earlier wave batch planned on the model;
    ``retry``: the test expects the call to roll back (the all-in-LDS form then gives way to the next one)."""
    cus = ctx.device_info()["n_cu"]
    wave = model != "lane" and n_actions <= 64
    if not wave:
        return "saopd_lane" + ("_retry" if retry else "")
    k = budget // n_actions
    need = nodes_before + 1 + k * n_actions
    tables = 3 * min(k + 3, 2560) * 8 + 128 * 4
    lds_qcap = 4096
    while lds_qcap < 2 * (1 + k * n_actions) and lds_qcap < (1 << 20):
        lds_qcap <<= 1
    if queue is not None:
        qcap = 2
        while qcap < queue:
            qcap <<= 1
        lds_qcap = min(lds_qcap, qcap)      # (a kept planner's queue only grows: the caller passes the size it has reached)
    lds_res = ((tables + 15) & ~15) + 16 + need * 36 + n_states * 20 + lds_qcap * 4
    fits = lds_res <= LDS_AVAIL
    use_lds = fits and (n_planners <= cus if lds is None else lds == "1")
    tab_lds = min(k + 3, (5 * 1024 - 32 - n_states * 40) // 24)
    use_dict = tab_lds >= 16 and (dictionary is None or dictionary == "1")
    if use_dict and lds is None:
        use_lds = False
    if device_arrays:
        use_lds = False
    if retry:
        use_lds = False
    ordered = (n_planners > 32 * cus if order is None else order == "1") and have_cost
    return "saopd_wave{}{}{}".format("_lds" if use_lds else "_dict" if use_dict else "", "_ordered" if ordered else "",
                                     "_retry" if retry else "")


def uct_stoch_form(records, path_bits, n_actions, policy=False, generic=False):
    """``records``: 0 rows and thresholds, 2 / 4 fused records, 1 compact records; ``path_bits`` 16 or 32; ``generic``:
    MP_UCT_STOCH_GENERIC_A=1."""
    unrolled = 2 <= n_actions <= 8 and not generic
    return "uct_stoch_r{}_p{}_a{}{}".format(records, path_bits, n_actions if unrolled else "any", "_policy" if policy else "")
