"""MDP-GapE with several next states per chance node (``max_next_states_count`` K >= 1) on deterministic, dense and sparse
finite-MDP models, restated in plain Python + numpy, for the tests only.

Reference: ``rl_agents/agents/tree_search/mdp_gape.py`` (run, plan, DecisionNode, ChanceNode with its placeholder children and
``backup_to_root``), ``olop.py:132-142`` (OLOPNode.update) and ``rl_agents/utils.py:150-203, 279-342`` (newton_iteration,
theta_func, d_theta_dl_func, max_expectation_under_constraint).  It calls numpy's own ``log``, ``exp`` and ``@`` on the arrays
the reference builds, so it is pinned on the reference's outputs BIT FOR BIT (tests/golden/gape_stoch.npz,
tests/golden/gape_transition.npz, tests/test_gape_stoch_host.py).  The decision nodes' KL bounds, the thresholds by count, the
initial values and best-arm identification are those of tests/gape_restatement.py.

What is new against one next state:

* the clone is re-seeded per episode with one draw ``x`` of the planner's generator: its generator is
  ``Generator(PCG64(SeedSequence(x)))`` and every step of a dense / sparse model is one ``choice(W, p=row)`` of it; a
  deterministic table draws nothing;
* a chance node gets K placeholder decision children at its first ``get_child``; an observation that is not among the children
  takes the lowest-numbered placeholder left (ValueError when none is), and Python's dict moves it to the END: the children are
  the placeholders left, in number order, then the observed states in the order they were first seen;
* a chance node's two values are ``p @ next`` for the ``p`` that :func:`max_expectation` finds around the empirical next-state
  frequencies, once for ``u_next`` and once for ``-l_next``.

The tree is kept as creation-order arrays over both kinds of node, the layout of tests/gape_restatement.py.  The ``action`` of a
decision node is the observed state, or ``-1 - i`` while it still is ``placeholder_i``; ``children`` keeps each node's children
in the reference's dict order, which :func:`as_bfs` follows.
"""
import math

import numpy as np

from tests.gape_restatement import CHANCE, DECISION, TREE_KEYS, bai, kl_bound_traced, value_init

# what max_expectation did, for the trace of mp_selftest_gape_transition (kl_transition.hpp holds the same values)
KT_UNIFORM_Q = 1        # q was all zeros and became uniform
KT_FSTAR_ABOVE = 2      # the largest f sits on a zero-probability entry: f_star > amax(f_p)
KT_ZERO_MASS = 4        # ... and theta_star < 0: mass z on the zero-probability maxima, lambda = f_star
KT_ISCLOSE = 8          # every f_p within numpy's isclose of the first: q is returned
KT_NEWTON = 16          # lambda from the Newton iteration
KT_CLAMP = 32           # an iterate fell below a = f_star and was pulled back (weight 0.9)
KT_FINAL_CLAMP = 64     # the last iterate was below a
KT_BETA_ZERO = 128      # beta == 0
KT_BETA_UNIFORM = 256   # ... and the mass went to the positive-probability maxima

NEWTON_EPS, NEWTON_WEIGHT, NEWTON_MAX_ITERATIONS = 1e-2, 0.9, 100
ISCLOSE_RTOL, ISCLOSE_ATOL = 1e-5, 1e-8


def max_expectation(f, q, c, log=np.log, exp=np.exp, observe=None):
    """argmax over p of E_p[f] subject to KL(q || p) <= c (utils.py:292-342) -> (p_star, Newton iterations, KT_* mask).
    numpy semantics throughout: a division by zero gives inf, an invalid operation NaN, nothing raises.
    ``observe(kind, a, b)``: every pair of numbers a comparison decides on."""
    observe = observe or (lambda kind, a, b: None)
    f, q = np.asarray(f, np.float64), np.asarray(q, np.float64)
    mask, iterations = 0, 0
    with np.errstate(all="ignore"):
        if np.all(q == 0):
            q = np.ones(q.size) / q.size
            mask |= KT_UNIFORM_Q
        plus, zero = q > 0, q == 0
        p_star = np.zeros(q.shape)
        q_p, f_p = q[plus], f[plus]
        f_star = np.amax(f)
        lam, z = None, 0

        def theta(x):
            d = x - f_p
            return q_p @ log(d) + log(q_p @ (1 / d)) - c

        def d_theta(x):
            inv = 1 / (x - f_p)
            s1 = q_p @ inv
            return s1 - (q_p @ (inv ** 2)) / s1

        observe("f_star", f_star, np.amax(f_p))
        if f_star > np.amax(f_p):
            mask |= KT_FSTAR_ABOVE
            theta_star = theta(f_star)
            observe("theta_star", theta_star, 0.0)
            if theta_star < 0:
                mask |= KT_ZERO_MASS
                lam = f_star
                z = 1 - exp(theta_star)
                top = 1.0 * (f[zero] == np.amax(f[zero]))
                p_star[zero] = top * (z / top.sum())
        if lam is None:
            for v in f_p:
                if np.isfinite(v) and np.isfinite(f_p[0]):
                    observe("isclose", abs(v - f_p[0]), ISCLOSE_ATOL + ISCLOSE_RTOL * abs(f_p[0]))
            if np.isclose(f_p, f_p[0]).all():
                return q, 0, mask | KT_ISCLOSE
            mask |= KT_NEWTON
            a = f_star
            x, x_next = np.inf, f_star + 1
            while abs(x - x_next) > NEWTON_EPS and iterations < NEWTON_MAX_ITERATIONS:
                iterations += 1
                x = x_next
                f_x, df_x = theta(x), d_theta(x)
                if df_x != 0:
                    x_next = x - f_x / df_x
                observe("below_a", x_next, a)
                if x_next < a:
                    x_next = NEWTON_WEIGHT * a + (1 - NEWTON_WEIGHT) * x
                    mask |= KT_CLAMP
                observe("eps", abs(x - x_next), NEWTON_EPS)
            if x_next < a:
                x_next = a
                mask |= KT_FINAL_CLAMP
            lam = x_next
        beta = (1 - z) / (q_p @ (1 / (lam - f_p)))
        observe("beta", beta, 0.0)
        if beta == 0:
            mask |= KT_BETA_ZERO
            uni = (q > 0) & (f == f_star)
            if uni.sum() > 0:
                mask |= KT_BETA_UNIFORM
                p_star[uni] = (1 - z) / uni.sum()
        else:
            p_star[plus] = beta * q_p / (lam - f_p)
    return p_star, iterations, mask


def transition_thresholds_by_count(expression, horizon, actions, confidence, episodes):
    """``transition_threshold()`` by the chance node's count 1 .. episodes + 2 (mdp_gape.py:307-313); the caller divides by
    the count."""
    time = episodes  # noqa: F841
    out = np.empty(int(episodes) + 2, np.float64)
    for count in range(1, int(episodes) + 3):
        out[count - 1] = float(eval(expression, {"np": np}, dict(horizon=horizon, actions=actions, confidence=confidence,
                                                                 count=count, time=time)))
    return out


def gape_stoch_plan(mode, transition, reward, terminal, s0, episodes, horizon, gamma, accuracy, thr_by_count, tthr_by_count,
                    max_next_states, continuation, rng, next_states=None, available=None, order=None, done_rule="source",
                    log=np.log, exp=np.exp, observe=None):
    """One MDPGapE.plan from state ``s0`` on a ``mode`` "deterministic" [S, A], "stochastic" [S, A, S] or "sparse" [S, A, B]
    model.  ``rng``: the planner's numpy Generator (advanced in place).  ``thr_by_count`` / ``tthr_by_count``: the reward
    bound's and the transition bound's threshold by count, ``[count - 1]``.  ``observe(kind, values)`` as
    ``gape_restatement.gape_plan``; the pairs :func:`max_expectation` compares arrive as ("transition/<kind>", [a, b]).
    Returns dict(plan, best, challenger, episodes_run, env_steps, error, children, kind, parent, action, depth, count, cum,
    mu_ucb, mu_lcb, vu, vl, done, state); ``error``: None, "one_action", "range" or "placeholders"."""
    observe = observe or (lambda kind, values: None)
    transition = np.asarray(transition)
    reward = np.asarray(reward, np.float64)
    term = np.zeros(reward.shape[0], bool) if terminal is None else np.asarray(terminal).astype(bool).reshape(-1)
    nxt = np.asarray(next_states) if mode == "sparse" else None
    n_actions, K = reward.shape[1], int(max_next_states)
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
        return kids[sel], kids[best], kids[chal]

    def transition_pairs(kind, a, b):
        observe("transition/" + kind, [float(a), float(b)])

    new_node(DECISION, -1, -1, 0, s0)
    env_steps, error, best, chal, episodes_run = 0, None, None, None, 0
    for episode in range(int(episodes) + 2):
        x = int(rng.integers(2 ** 30))
        clone = None if mode == "deterministic" else np.random.Generator(np.random.PCG64(np.random.SeedSequence(x)))
        if not children[0]:
            expand(0)
        node, path = 0, [0]
        for h in range(int(horizon)):
            s = T["state"][node]
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
                chance = kids[int(rng.choice(ties))]
            else:
                act = int(rng.integers(n_actions)) if continuation == "uniform" else 0
                expand(node)
                match = [c for c in children[node] if T["action"][c] == act]
                chance = match[0] if match else children[node][0]
            act = T["action"][chance]
            r = float(reward[s, act])
            if mode == "deterministic":
                s_next = int(transition[s, act])
            else:
                b = int(clone.choice(transition.shape[2], p=transition[s, act]))
                s_next = int(nxt[s, act, b]) if nxt is not None else b
            d = bool(term[s] if done_rule == "source" else term[s_next])
            env_steps += 1
            # ChanceNode.get_child: the placeholders, then the observation among the children or the first placeholder left
            if not children[chance]:
                for i in range(K):
                    children[chance].append(new_node(DECISION, chance, -1 - i, T["depth"][chance] + 1, -1))
            match = [c for c in children[chance] if T["action"][c] == s_next]
            if match:
                dec = match[0]
            else:
                left = [c for c in children[chance] if T["action"][c] < 0]
                if not left:
                    error = "placeholders"
                    break
                dec = left[0]
                children[chance].remove(dec)
                children[chance].append(dec)
                T["action"][dec] = T["state"][dec] = s_next
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
        for n in reversed(path):
            if T["kind"][n] == DECISION:
                if children[n]:
                    T["vu"][n] = float(np.amax([T["vu"][c] for c in children[n]]))
                    T["vl"][n] = float(np.amax([T["vl"][c] for c in children[n]]))
                else:
                    T["vu"][n] = T["vl"][n] = 0.0
            else:
                kids = children[n]
                u_next = np.array([T["mu_ucb"][c] + gamma * T["vu"][c] for c in kids])
                l_next = np.array([T["mu_lcb"][c] + gamma * T["vl"][c] for c in kids])
                p_hat = np.array([T["count"][c] for c in kids]) / T["count"][n]
                threshold = tthr_by_count[T["count"][n] - 1] / T["count"][n]
                p_plus = max_expectation(u_next, p_hat, threshold, log, exp, transition_pairs)[0]
                p_minus = max_expectation(-l_next, p_hat, threshold, log, exp, transition_pairs)[0]
                T["vu"][n] = float(p_plus @ u_next)
                T["vl"][n] = float(p_minus @ l_next)
        _, best, chal = root_bai()
        episodes_run = episode + 1
        observe("stop", [T["vu"][chal] - T["vl"][best], accuracy])
        if T["vu"][chal] - T["vl"][best] < accuracy or episode > episodes:
            break
    out = dict(plan=np.asarray([] if error else [T["action"][best]], np.int32), error=error, env_steps=env_steps,
               episodes_run=episodes_run, best=-1 if error else T["action"][best], challenger=-1 if error else T["action"][chal],
               children=children)
    dt = dict(kind=np.uint8, parent=np.int32, action=np.int32, depth=np.int32, count=np.int64, done=np.uint8, state=np.int32)
    out.update({k: np.asarray(v, dt.get(k, np.float64)) for k, v in T.items()})
    return out


def as_bfs(tree):
    """A creation-order tree of :func:`gape_stoch_plan` -> the golden BFS listing: children in the reference's dict order,
    ``parent`` = the BFS position."""
    order, i = [0], 0
    while i < len(order):
        order.extend(tree["children"][order[i]])
        i += 1
    order = np.asarray(order, np.int64)
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    out = {k: np.asarray(tree[k])[order] for k in TREE_KEYS if k in tree}
    par = np.asarray(tree["parent"])[order]
    out["parent"] = np.where(par >= 0, pos[np.maximum(par, 0)], -1).astype(np.int32)
    return out


def smallest_margin(pairs):
    """The smallest distance between two compared numbers that are not equal (inf when there is none)."""
    d = [abs(a - b) for a, b in pairs if a != b and math.isfinite(a) and math.isfinite(b)]
    return min(d) if d else math.inf
