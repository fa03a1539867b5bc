"""Sparse Sampling restated in plain Python + numpy, for the tests only.

Reference: ``rl_agents/agents/tree_search/sparse_sampling.py:21-28`` (plan, get_plan) with its nodes (:31-96), on a
deterministic, dense stochastic or sparse finite-MDP table.  Its job is to let GPU tests check random cases and sampled roots
of big batches against something other than the kernel; it is itself pinned on the reference's own outputs
(tests/golden/sparse_sampling.npz, tests/test_sparse_sampling_host.py).  numpy's own ``Generator`` and ``SeedSequence`` draw.

The tree is kept as creation-order arrays, the layout of ``mp_ss_tree_export``.
"""
import numpy as np

TREE_KEYS = ("parent", "key", "is_chance", "depth", "count", "value")


def listed_actions(n_actions, s, available=None, order=None):
    """``state.get_available_actions()`` in the env's listing order, or ``range(n)`` for an env without it (:40-43)."""
    seq = range(n_actions) if order is None else [int(a) for a in order]
    return [a for a in seq if available is None or available[s, a]]


def max_outdegree(mode, transition):
    """W: the most outcomes one (state, action) can give."""
    if mode == "deterministic":
        return 1
    t = np.asarray(transition)
    return int(t.shape[2]) if mode == "sparse" else int(np.count_nonzero(t, axis=2).max())


def node_bound(n_actions, horizon, width):
    """D_0 = 1 decision node, |A| D_d chance nodes at depth d, D_(d+1) <= |A| D_d width."""
    dec, total = 1, 1
    for _ in range(horizon):
        chance = n_actions * dec
        dec = chance * width
        total += chance + dec
    return total


def ss_plan(mode, transition, reward, s0, horizon, n_samples, gamma, rng, nxt=None, available=None, order=None):
    """One SparseSampling.plan from state ``s0``.  ``rng``: a numpy Generator (advanced in place).  Returns creation-order
    arrays (parent, key, is_chance, depth, count, value), the plan, the root's chance values with their actions in listing
    order, ``samples`` (model steps) -- or ``error`` = "empty" where the reference raises ValueError (horizon 0: :55)."""
    transition, reward = np.asarray(transition), np.asarray(reward, dtype=np.float64)
    n_actions = reward.shape[1]
    parent, key, is_chance, depth, count, value, children = [-1], [-1], [0], [0], [0], [0], [{}]
    samples = [0]

    def child(node, k, chance):
        kids = children[node]
        if k not in kids:
            kids[k] = len(parent)
            parent.append(node); key.append(k); is_chance.append(1 if chance else 0)
            depth.append(depth[node] if chance else depth[node] + 1)       # :34, :68
            count.append(0); value.append(0); children.append({})
        return kids[k]

    def step(s, a, x):
        """A clone seeded with ``x`` steps once (FiniteMDPEnv.seed / step): the draw is made for every model."""
        env_gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(x))))
        r = float(reward[s, a])
        if mode == "deterministic":
            return int(transition[s, a]), r
        b = int(env_gen.choice(transition.shape[2], p=transition[s, a]))
        return (b if mode == "stochastic" else int(nxt[s, a, b])), r

    def estimate_v(node, s):                                               # :38-51
        if depth[node] == horizon:
            return
        for a in listed_actions(n_actions, s, available, order):
            estimate_q(child(node, a, True), s, a)
        value[node] = np.amax([value[c] for c in children[node].values()])

    def estimate_q(node, s, a):                                            # :71-88
        if depth[node] == horizon:
            return
        for _ in range(n_samples):
            sn, r = step(s, a, rng.integers(2 ** 30))
            samples[0] += 1
            count[child(node, sn, False)] += 1
        for sn, c in list(children[node].items()):
            estimate_v(c, sn)
        value[node] = r + gamma * sum(value[c] * count[c] for c in children[node].values()) / n_samples

    estimate_v(0, int(s0))
    out = dict(parent=np.asarray(parent, np.int32), key=np.asarray(key, np.int32), is_chance=np.asarray(is_chance, np.uint8),
               depth=np.asarray(depth, np.int32), count=np.asarray(count, np.int64),
               value=np.asarray([float(v) for v in value], np.float64), samples=samples[0], error=None, plan=None,
               root_actions=np.asarray(list(children[0].keys()), np.int32),
               root_values=np.asarray([float(value[c]) for c in children[0].values()], np.float64), root_value=0.0)
    if not children[0]:
        out["error"] = "empty"                                             # np.amax([]) raises ValueError
        return out
    values = out["root_values"]
    ties = np.nonzero(values == np.amax(values))[0]                        # abstract.py:296-311
    pick = int(rng.choice(ties))
    out["plan"] = np.asarray([out["root_actions"][pick]], np.int32)
    out["root_value"] = float(values[pick])
    return out


def as_bfs(tree):
    """Creation-order arrays -> the BFS listing of the goldens (children in creation order)."""
    n = len(tree["parent"])
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[int(tree["parent"][i])].append(i)
    order, i = [0], 0
    while i < len(order):
        order.extend(kids[order[i]])
        i += 1
    new = np.empty(n, np.int64)
    new[order] = np.arange(n)
    out = {k: np.asarray(tree[k])[order] for k in TREE_KEYS}
    out["parent"] = np.asarray([-1 if p < 0 else new[p] for p in out["parent"]], np.int32)
    return out


def half_words(record, n):
    """The next ``n`` 32-bit draws of a six-word PCG64 record, from the raw 64-bit stream: the buffered half first when the
    record holds one, then the low and the high half of every output."""
    from numpy.random import PCG64
    bg = PCG64()
    st = bg.state
    st["state"] = {"state": (int(record[0]) << 64) | int(record[1]), "inc": (int(record[2]) << 64) | int(record[3])}
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    words = [int(record[5])] if int(record[4]) else []
    raw = bg.random_raw((n + 1) // 2 + 1)
    for o in raw:
        words += [int(o) & 0xffffffff, int(o) >> 32]
    return words[:n]
