"""MDP-GapE on a deterministic finite-MDP table (``max_next_states_count == 1``) restated in plain Python + numpy, for the
tests only.

Reference: ``rl_agents/agents/tree_search/mdp_gape.py`` (run, plan, DecisionNode, ChanceNode), ``olop.py:132-142``
(OLOPNode.update) and ``rl_agents/utils.py:123-203`` (kl_upper_bound with ``lower``, newton_iteration).  It is pinned on the
reference's own outputs (tests/golden/gape.npz, tests/test_gape_host.py; the lower bound alone on
tests/golden/kl_lower_bound.npz) and lets the GPU tests check batches against something other than the kernel.

With one next state per chance node ``p_hat == [1.0]`` and ``max_expectation_under_constraint`` returns it
(utils.py:325-326), so a chance node's values are ``mu + gamma * value`` of its one decision child.

The tree is kept as creation-order arrays over BOTH kinds of node, the layout of ``mp_gape_tree_export``: ``kind`` 0 a decision
node (``action`` = the observed state, -1 at the root), 1 a chance node (``action`` = the action id; its depth is its
parent's).  A chance node carries no reward statistics: ``cum``, ``mu_ucb``, ``mu_lcb`` and ``done`` are 0 there.
"""
import math

import numpy as np

from tests.olop_restatement import (KL_CLAMP_LOWER, KL_CLAMP_UPPER, KL_EPS, KL_FINAL_LOWER, KL_FINAL_UPPER, KL_FINITE_DIFFERENCE,
                                    KL_MAX_ITERATIONS, KL_WEIGHT, _bernoulli_kl, bfs_order)

DECISION, CHANCE = 0, 1
DEFAULT_THRESHOLD = "3*np.log(1 + np.log(count))+ horizon*np.log(actions)+ np.log(1/(1-confidence))"


def kl_bound_traced(total, count, threshold, lower=False, log=np.log):
    """utils.py:123-147 with newton_iteration (:150-203) for either side: ``lower`` solves on [0, mu] from mu / 2, else on
    [mu, 1] from (mu + 1) / 2.  ``py_x`` tracks whether the iterate is still a Python float, as
    ``olop_restatement.kl_upper_bound_traced`` does: x0 is one (a sum of Python numbers halved), a Newton step makes a numpy
    scalar (f(x) went through np.log), a clamp ``weight * a + (1 - weight) * x`` keeps the kind of x.
    Returns (bound, Newton iterations, mask of the decisions taken)."""
    if count == 0:
        return (0.0 if lower else 1.0), 0, 0
    mu = total / count
    max_div = threshold / count
    a, b = (0.0, mu) if lower else (mu, 1.0)
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


def jittered_log(seed, ulps=2):
    """``np.log`` moved by up to ``ulps`` units in the last place, seeded: what another libm may return."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def log(x):
        y = np.float64(np.log(x))
        k = int(rng.integers(-ulps, ulps + 1))
        if not np.isfinite(y):
            return y
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        return y
    return log


def thresholds_by_count(expression, horizon, actions, confidence, episodes):
    """The bound's threshold by the node's count 1 .. episodes + 2 (mdp_gape.py:200-208): ``eval`` of the config string with
    the reference's variable names.  What the eval raises is raised."""
    time = episodes  # noqa: F841
    out = np.empty(int(episodes) + 2, np.float64)
    for count in range(1, int(episodes) + 3):
        out[count - 1] = float(eval(expression, {"np": np}, dict(horizon=horizon, actions=actions, confidence=confidence,
                                                                 count=count, time=time)))
    return out


def value_init(gamma, horizon):
    """A new node's value_upper by depth 0..horizon (mdp_gape.py:147, :258), in Python arithmetic."""
    return np.array([(1 - gamma ** (horizon - d)) / (1 - gamma) for d in range(int(horizon) + 1)], np.float64)


def bai(vu, vl):
    """best_arm_identification_selection (mdp_gape.py:228-249) on the children's bounds in order -> (selected, best,
    challenger) positions; ValueError with one child, as the reference's max() of an empty list."""
    n = len(vu)
    gaps = []
    for i in range(n):
        gap = -math.inf
        for j in range(n):
            if j != i:
                gap = max(gap, vu[j] - vl[i])
        gaps.append(gap)
    best = min(range(n), key=lambda i: gaps[i])
    challenger = max([i for i in range(n) if i != best], key=lambda i: vu[i])
    selected = max([best, challenger], key=lambda i: vu[i] - vl[i])
    return selected, best, challenger, gaps


def gape_plan(transition, reward, terminal, s0, episodes, horizon, gamma, accuracy, thr_by_count, continuation, rng,
              available=None, order=None, done_rule="source", log=np.log, observe=None):
    """One MDPGapE.plan from state ``s0``.  ``rng``: a numpy Generator (advanced in place).  ``thr_by_count``: the bound's
    threshold by count, ``thr_by_count[count - 1]``.  ``continuation``: "uniform" draws over ALL action ids at a childless
    node, anything else takes action 0; an action that is not listed there gives way to the first listed one.
    ``observe(kind, values)``: called with every set of numbers the planner compares (for the margin checks), and with what
    the sweep's contents are read from: "ties" [size of the tie set, rank drawn in it, position drawn among the children] and
    "continuation" [action drawn, 1 if listed else 0, its column in the listing order]; "arms" [the positions among the root's
    children of the best arm, the challenger, the selected one, the first largest and the first second-largest value_upper].
    Returns dict(plan, best, challenger, episodes_run, env_steps, error, kind, parent, action, depth, count, cum, mu_ucb,
    mu_lcb, vu, vl, done, state)."""
    observe = observe or (lambda kind, values: None)
    transition = np.asarray(transition)
    reward = np.asarray(reward, np.float64)
    term = np.zeros(reward.shape[0], bool) if terminal is None else np.asarray(terminal).astype(bool).reshape(-1)
    n_actions = reward.shape[1]
    order = list(range(n_actions)) if order is None else [int(a) for a in order]
    vinit = value_init(gamma, horizon)
    T = dict(kind=[], parent=[], action=[], depth=[], count=[], cum=[], mu_ucb=[], mu_lcb=[], vu=[], vl=[], done=[], state=[])
    children = []

    def new_node(kind, p, key, d, s):
        T["kind"].append(kind); T["parent"].append(p); T["action"].append(key); T["depth"].append(d); T["count"].append(0)
        T["cum"].append(0.0); T["mu_ucb"].append(1.0 if kind == DECISION else 0.0); T["mu_lcb"].append(0.0)
        T["vu"].append(float(vinit[d])); T["vl"].append(0.0); T["done"].append(False); T["state"].append(int(s))
        children.append([])
        return len(children) - 1

    def expand(node):
        s = T["state"][node]
        for a in order:
            if available is None or available[s, a]:
                children[node].append(new_node(CHANCE, node, a, T["depth"][node], s))

    def root_bai():
        kids = children[0]
        if len(kids) < 2:
            raise ValueError("max() arg is an empty sequence")
        sel, best, chal, gaps = bai([T["vu"][c] for c in kids], [T["vl"][c] for c in kids])
        observe("gaps", gaps)
        observe("challenger", [T["vu"][c] for i, c in enumerate(kids) if i != best])
        observe("widths", [T["vu"][kids[i]] - T["vl"][kids[i]] for i in (best, chal)])
        ups = [T["vu"][c] for c in kids]
        top1 = max(range(len(kids)), key=lambda i: ups[i])
        observe("arms", [best, chal, sel, top1, max([i for i in range(len(kids)) if i != top1], key=lambda i: ups[i])])
        return kids[sel], kids[best], kids[chal]

    new_node(DECISION, -1, -1, 0, s0)
    env_steps, error, best, chal, episodes_run = 0, None, None, None, 0
    for episode in range(int(episodes) + 2):
        rng.integers(2 ** 30)
        if not children[0]:
            expand(0)
        node, path = 0, [0]
        for h in range(int(horizon)):
            s = T["state"][node]
            # sampling_rule
            if node == 0:
                try:
                    chance = root_bai()[0]
                except ValueError:
                    error = "one_action"
                    break
            elif children[node]:
                kids = children[node]
                ups = np.array([T["vu"][c] for c in kids])
                observe("argmax", ups.tolist())
                ties = np.flatnonzero(ups == np.amax(ups))
                pick = int(rng.choice(ties))
                observe("ties", [len(ties), int(np.searchsorted(ties, pick)), pick])
                chance = kids[pick]
            else:
                act = int(rng.integers(n_actions)) if continuation == "uniform" else 0
                expand(node)
                match = [c for c in children[node] if T["action"][c] == act]
                observe("continuation", [act, 1 if match else 0, order.index(act) if act in order else -1])
                chance = match[0] if match else children[node][0]
            act = T["action"][chance]
            r = float(reward[s, act])
            s_next = int(transition[s, act])
            d = bool(term[s] if done_rule == "source" else term[s_next])
            env_steps += 1
            if not children[chance]:
                children[chance].append(new_node(DECISION, chance, s_next, T["depth"][chance] + 1, s_next))
            dec = children[chance][0]
            T["count"][chance] += 1
            if not 0 <= r <= 1:
                error = "range"
                break
            if d:
                T["done"][dec] = True
            if T["done"][dec]:
                r = 0
            T["cum"][dec] += r
            T["count"][dec] += 1
            thr = thr_by_count[T["count"][dec] - 1]
            T["mu_ucb"][dec] = float(kl_bound_traced(T["cum"][dec], T["count"][dec], thr, False, log)[0])
            T["mu_lcb"][dec] = float(kl_bound_traced(T["cum"][dec], T["count"][dec], thr, True, log)[0])
            path += [chance, dec]
            node = dec
        if error:
            break
        # backup_to_root
        for n in reversed(path):
            if T["kind"][n] == DECISION:
                if children[n]:
                    T["vu"][n] = float(np.amax([T["vu"][c] for c in children[n]]))
                    T["vl"][n] = float(np.amax([T["vl"][c] for c in children[n]]))
                else:
                    T["vu"][n] = T["vl"][n] = 0.0
            else:
                c = children[n][0]
                T["vu"][n] = float(T["mu_ucb"][c] + gamma * T["vu"][c])
                T["vl"][n] = float(T["mu_lcb"][c] + gamma * T["vl"][c])
        _, best, chal = root_bai()
        episodes_run = episode + 1
        observe("stop", [T["vu"][chal] - T["vl"][best], accuracy])
        if T["vu"][chal] - T["vl"][best] < accuracy or episode > episodes:
            break
    out = dict(plan=np.asarray([] if error else [T["action"][best]], np.int32), error=error, env_steps=env_steps,
               episodes_run=episodes_run, best=-1 if error else T["action"][best], challenger=-1 if error else T["action"][chal])
    dt = dict(kind=np.uint8, parent=np.int32, action=np.int32, depth=np.int32, count=np.int64, done=np.uint8, state=np.int32)
    out.update({k: np.asarray(v, dt.get(k, np.float64)) for k, v in T.items()})
    return out


TREE_KEYS = ("kind", "action", "depth", "count", "cum", "mu_ucb", "mu_lcb", "vu", "vl", "done", "state")


def as_bfs(tree):
    """A creation-order tree dict -> the golden BFS listing (children in creation order; parent = BFS position)."""
    order = bfs_order(tree["parent"])
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    out = {k: np.asarray(tree[k])[order] for k in TREE_KEYS if k in tree}
    par = np.asarray(tree["parent"])[order]
    out["parent"] = np.where(par >= 0, pos[np.maximum(par, 0)], -1).astype(np.int32)
    return out
