"""OLOP / KL-OLOP restated in plain Python + numpy, for the tests only.

Reference: ``rl_agents/agents/tree_search/olop.py:64-193`` (run, OLOPNode.update / compute_reward_ucb / expand /
backup_to_root, selection_rule) and ``rl_agents/utils.py:89-203`` (kl_upper_bound, newton_iteration), on a deterministic
finite-MDP table.  Its job is to let GPU tests check random cases and sampled roots of big batches against something
other than the kernel; it is itself pinned on the reference's own outputs (tests/golden/olop.npz, tests/test_olop_host.py;
the bound alone on tests/golden/kl_bound.npz and plans with NaN bounds on tests/golden/olop_nan.npz, tests/test_olop_bound_host.py).

The tree is kept as creation-order arrays, the layout of ``mp_olop_tree_export``.
"""
import math

import numpy as np

KL_EPS = 1e-2
KL_WEIGHT = 0.9
KL_MAX_ITERATIONS = 100


# decisions of one kl_upper_bound evaluation, the bit mask of mp_selftest_olop_bound
KL_CLAMP_UPPER, KL_CLAMP_LOWER, KL_FINITE_DIFFERENCE, KL_FINAL_LOWER, KL_FINAL_UPPER = 1, 2, 4, 8, 16


def _bernoulli_kl(p, q, log=np.log):
    """KL(B(p) || B(q)) with the case analysis of utils.py:89-109 (numpy's log on the host)."""
    head = p * log(p / q) if (p > 0 and q > 0) else 0.0
    if not q < 1:
        tail = math.inf
    else:
        tail = (1 - p) * log((1 - p) / (1 - q)) if p < 1 else 0.0
    return float(head + tail)


def kl_upper_bound_traced(total, count, threshold, log=np.log):
    """utils.py:123-146 with newton_iteration (:149-203), eps 1e-2, weight 0.9, 100 iterations.  ``py_x`` tracks whether
    the iterate is still a Python float (the first derivative then raises ZeroDivisionError instead of giving inf).
    Returns (bound, Newton iterations, mask of the decisions taken: KL_* above); ``log`` replaces numpy's, for tests that
    move it by an ulp or record its arguments."""
    if count == 0:
        return 1.0, 0, 0
    mu = total / count
    max_div = threshold / count
    a, b = mu, 1.0
    x0 = (a + b) / 2
    if a == b:
        return a, 0, 0
    decisions = 0
    with np.errstate(all="ignore"):
        x, x_next, py_next = math.inf, x0, True
        iterations = 0
        while abs(x - x_next) > KL_EPS and iterations < KL_MAX_ITERATIONS:
            iterations += 1
            x, py_x = x_next, py_next
            f_x = _bernoulli_kl(mu, x, log) - max_div
            if py_x and (1 - x == 0 or x == 0):
                df_x = (f_x - (_bernoulli_kl(mu, x - KL_EPS, log) - max_div)) / KL_EPS
                decisions |= KL_FINITE_DIFFERENCE
            else:
                df_x = float(np.float64(1 - mu) / np.float64(1 - x) - np.float64(mu) / np.float64(x))
            if df_x != 0:
                x_next = float(np.float64(x) - np.float64(f_x) / np.float64(df_x))
                py_next = False
            if x_next < a:
                x_next, py_next = KL_WEIGHT * a + (1 - KL_WEIGHT) * x, py_x
                decisions |= KL_CLAMP_LOWER
            elif x_next > b:
                x_next, py_next = KL_WEIGHT * b + (1 - KL_WEIGHT) * x, py_x
                decisions |= KL_CLAMP_UPPER
    if x_next < a:
        x_next = a
        decisions |= KL_FINAL_LOWER
    if x_next > b:
        x_next = b
        decisions |= KL_FINAL_UPPER
    return x_next, iterations, decisions


def kl_upper_bound(total, count, threshold):
    return kl_upper_bound_traced(total, count, threshold)[0]


def thresholds(expression, time_ref, episodes):
    """The bound's threshold per episode (olop.py:145-158): ``eval`` of the config string with ``time`` = episodes
    (global) or episode + 1 (local)."""
    out = np.empty(max(int(episodes), 1), np.float64)
    for e in range(int(episodes)):
        time = episodes if time_ref == "global" else (e + 1 if time_ref == "local" else np.nan)  # noqa: F841
        out[e] = float(eval(expression, {"np": np, "time": time}))
    return out[:int(episodes)]


def value_upper_init(gamma, horizon):
    return np.array([(1 - gamma ** (horizon + 1 - d)) / (1 - gamma) for d in range(horizon + 1)], np.float64)


def _first_max(values):
    """Python ``max`` over the list with ``>`` (the first element stays when nothing exceeds it, a NaN included)."""
    best, idx = values[0], 0
    for i in range(1, len(values)):
        if values[i] > best:
            best, idx = values[i], i
    return idx


def olop_plan(transition, reward, terminal, s0, episodes, horizon, gamma, kl, thr, continuation, rng,
              available=None, order=None, done_rule="source", first_max=None, amax=np.amax):
    """One OLOP.plan from state ``s0``.  ``rng``: a numpy Generator (advanced in place).  ``thr``: per-episode thresholds.
    ``available`` [S, A] bool and ``order`` (listing order of the action ids) as ``get_available_actions`` lists them.
    ``first_max`` / ``amax``: other rules in place of Python's ``max`` (olop.py:84, :126-130) and ``np.amax`` (:188), for tests
    that show which cases tell a wrong NaN rule from the right one.
    Returns dict(plan, parent, action, depth, count, cum, mu, vu, done, state, env_steps, error)."""
    first_max = first_max or _first_max
    transition = np.asarray(transition)
    reward = np.asarray(reward, np.float64)
    term = np.zeros(reward.shape[0], bool) if terminal is None else np.asarray(terminal).astype(bool).reshape(-1)
    n_actions = reward.shape[1]
    order = list(range(n_actions)) if order is None else [int(a) for a in order]
    vinit = value_upper_init(gamma, horizon)
    mu0 = 1.0 if kl else math.inf
    parent, action, depth, count, cum, mu, vu, done, state, children = [], [], [], [], [], [], [], [], [], []

    def new_node(p, a, d, s):
        parent.append(p); action.append(a); depth.append(d); count.append(0); cum.append(0.0)
        mu.append(mu0); vu.append(float(vinit[d])); done.append(False); state.append(int(s)); children.append([])
        return len(parent) - 1

    new_node(-1, -1, 0, s0)
    env_steps, error = 0, None
    for e in range(int(episodes)):
        rng.integers(2 ** 30)
        node, path = 0, [0]
        for h in range(int(horizon)):
            s = state[node]
            if not children[node]:
                acts = [a for a in order if available is None or available[s, a]]
                for a in acts:
                    children[node].append(new_node(node, a, depth[node] + 1, transition[s, a]))
                if continuation == "uniform":
                    act = int(rng.choice(acts))
                else:
                    act = 0
            else:
                kids = children[node]
                act = action[kids[first_max([vu[c] for c in kids])]]
            r = float(reward[s, act])
            s_next = int(transition[s, act])
            d = bool(term[s] if done_rule == "source" else term[s_next])
            env_steps += 1
            match = [c for c in children[node] if action[c] == act]
            if not match:
                error = "key"
                break
            node = match[0]
            if not 0 <= r <= 1:
                error = "range"
                break
            if d:
                done[node] = True
            if done[node]:
                r = 0
            cum[node] += r
            count[node] += 1
            if kl:
                mu[node] = kl_upper_bound(cum[node], count[node], thr[e])
            path.append(node)
        if error:
            break
        for n in reversed(path):
            if children[n]:
                m = amax([vu[c] for c in children[n]])
                vu[n] = float(mu[n] + gamma * m)
            else:
                vu[n] = mu[n]
    plan = []
    if error is None:
        node = 0
        while children[node]:
            kids = children[node]
            cnt = np.array([count[c] for c in kids])
            tops = np.flatnonzero(cnt == cnt.max())
            pick = kids[tops[first_max([vu[kids[i]] for i in tops])]]
            plan.append(action[pick])
            node = pick
    return dict(plan=np.asarray(plan, np.int32), parent=np.asarray(parent, np.int32), action=np.asarray(action, np.int32),
                depth=np.asarray(depth, np.int32), count=np.asarray(count, np.int64), cum=np.asarray(cum, np.float64),
                mu=np.asarray(mu, np.float64), vu=np.asarray(vu, np.float64), done=np.asarray(done, np.uint8),
                state=np.asarray(state, np.int32), env_steps=env_steps, error=error)


def bfs_order(parent):
    """Creation-order node ids in the golden files' BFS listing (children in creation order)."""
    parent = np.asarray(parent)
    kids = [[] for _ in range(len(parent))]
    for i in range(1, len(parent)):
        kids[parent[i]].append(i)
    order, i = [0], 0
    while i < len(order):
        order.extend(kids[order[i]])
        i += 1
    return np.asarray(order, np.int64)


def as_bfs(tree):
    """A creation-order tree dict -> the golden BFS listing (parent = BFS position of the parent)."""
    order = bfs_order(tree["parent"])
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    out = {k: np.asarray(tree[k])[order] for k in ("action", "depth", "count", "cum", "mu", "vu", "done", "state") if k in tree}
    par = np.asarray(tree["parent"])[order]
    out["parent"] = np.where(par >= 0, pos[np.maximum(par, 0)], -1).astype(np.int32)
    return out
