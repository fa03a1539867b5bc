"""BRUE restated in plain Python + numpy, for the tests only.

Reference: ``rl_agents/agents/tree_search/brue.py:24-75`` (rollout, update, estimate, plan, get_plan) with its nodes
(:78-116), on a deterministic, dense stochastic or sparse finite-MDP table.  Its job is to let GPU tests check random
cases and sampled roots of big batches against something other than the kernel; it is itself pinned on the reference's
own outputs (tests/golden/brue.npz, tests/test_brue_host.py).  numpy's own ``Generator`` and ``SeedSequence`` draw.

The tree is kept as creation-order arrays, the layout of ``mp_brue_tree_export``.
"""
import numpy as np


def env_step(mode, transition, nxt, reward, terminal, done_rule, s, a, env_gen):
    """FiniteMDPEnv.step: reward[s, a], the next state (one ``choice(..., p=row)`` of the env's generator on a stochastic
    / sparse row, nothing on a deterministic one), done by the model's rule."""
    r = float(reward[s, a])
    if mode == "deterministic":
        sn = int(transition[s, a])
    elif mode == "stochastic":
        sn = int(env_gen.choice(transition.shape[2], p=transition[s, a]))
    else:
        sn = int(nxt[s, a, int(env_gen.choice(transition.shape[2], p=transition[s, a]))])
    done = bool(terminal[s] if done_rule == "source" else terminal[sn])
    return sn, r, done


def brue_plan(mode, transition, reward, terminal, s0, budget, horizon, gamma, rng, nxt=None, done_rule="source"):
    """One BRUE.plan from state ``s0``.  ``rng``: a numpy Generator (advanced in place).  Returns creation-order arrays
    (parent, key, is_chance, depth, count, stat), the plan, env_steps, the value of the chosen chance node, how many
    children tied at the root -- or ``error`` = "empty" where the reference raises ValueError (no rollout: brue.py:75)."""
    transition, reward = np.asarray(transition), np.asarray(reward, dtype=np.float64)
    terminal = np.asarray(terminal).astype(bool)
    n_actions = reward.shape[1]
    parent, key, is_chance, depth, count, stat, children = [-1], [-1], [0], [0], [0], [0.0], [{}]

    def child(node, k, chance):
        kids = children[node]
        if k not in kids:
            kids[k] = len(parent)
            parent.append(node); key.append(k); is_chance.append(1 if chance else 0)
            depth.append(depth[node] if chance else depth[node] + 1)       # brue.py:81,103
            count.append(0); stat.append(0.0); children.append({})
        return kids[k]

    def update(node, x):                                                   # brue.py:84-86, 106-108
        count[node] += 1
        stat[node] = (count[node] - 1) / count[node] * stat[node] + x / count[node]

    def estimate(node):                                                    # brue.py:52-64
        ret = 0
        for d in range(horizon - depth[node]):
            if not children[node]:
                break
            kids = list(children[node].values())
            best = kids[0]
            for c in kids[1:]:                                             # Python max: the first maximum
                if stat[c] > stat[best]:
                    best = c
            outcomes = list(children[best].values())
            counts = np.array([count[c] for c in outcomes])
            node = outcomes[int(rng.choice(len(outcomes), p=counts / counts.sum()))]
            ret += gamma ** d * stat[node]
        return ret

    env_steps = 0
    available = budget
    while available > 0:
        env_gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(rng.integers(2 ** 30)))))
        s, node, todo = int(s0), 0, []
        for _ in range(horizon):                                           # brue.py:24-33
            a = int(rng.integers(n_actions))
            sn, r, done = env_step(mode, transition, nxt, reward, terminal, done_rule, s, a, env_gen)
            env_steps += 1
            chance = child(node, a, True)
            nxt_node = child(chance, sn, False)
            todo.append((chance, r, nxt_node))
            node, s = nxt_node, sn
            available -= 1
            if done:
                break
        for chance, r, nxt_node in reversed(todo):                         # brue.py:47-50
            update(nxt_node, r)
            update(chance, r + gamma * estimate(nxt_node))

    out = dict(parent=np.asarray(parent, np.int32), key=np.asarray(key, np.int32), is_chance=np.asarray(is_chance, np.uint8),
               depth=np.asarray(depth, np.int32), count=np.asarray(count, np.int64), stat=np.asarray(stat, np.float64),
               env_steps=env_steps, error=None, plan=None, root_value=0.0, ties=0)
    kids = list(children[0].values())
    if not kids:
        out["error"] = "empty"                                             # np.amax([]) raises ValueError
        return out
    values = np.asarray([stat[c] for c in kids])
    ties = np.nonzero(values == np.amax(values))[0]                        # abstract.py:296-311
    pick = int(rng.choice(ties))
    out["plan"] = np.asarray([key[kids[pick]]], np.int32)
    out["root_value"], out["ties"] = float(values[pick]), len(ties)
    return out


TREE_KEYS = ("parent", "key", "is_chance", "depth", "count", "stat")


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


def visits_of(tree):
    """planner.get_visits(): every model step is a visit of the decision node it led to (abstract.py:158-167)."""
    visits = {}
    for k, c, ch, p in zip(tree["key"], tree["count"], tree["is_chance"], tree["parent"]):
        if p >= 0 and not ch and c > 0:
            visits[str(int(k))] = visits.get(str(int(k)), 0) + int(c)
    return visits
