"""OLOP / KL-OLOP on a STOCHASTIC finite MDP restated in plain Python + numpy, for the tests only.

Reference: ``rl_agents/agents/tree_search/olop.py:64-193`` and ``rl_agents/utils.py:89-203`` on a ``stochastic`` [S, A, S] or
``sparse`` [S, A, B] model of this package's ``FiniteMDPEnv`` family.  The bound, the thresholds, the initial upper bounds and
Python's ``max`` come from tests/olop_restatement.py; what is restated here is what changes when the model is sampled:

* an episode re-seeds its clone with one draw ``x`` of the planner's generator (olop.py:73): the clone's generator is
  ``Generator(PCG64(SeedSequence(x)))`` and every model step is ONE ``choice(W, p=row)`` of it (finite_mdp.py);
* the state belongs to the episode, not to the node: an expansion lists the actions of the clone's CURRENT state, a node's
  children are fixed at its first expansion, and a later episode that reaches the node in another state steps the selected
  child whether or not that state lists its action;
* ``done`` is what the step reports (the done rule on the source or the next state) and sticks to the node.

It is pinned on the reference's own outputs (tests/golden/olop_stoch.npz, tests/test_olop_stoch_host.py).  The tree is kept as
creation-order arrays, the layout of ``mp_olop_tree_export``: ``state`` is the root's at node 0 and -1 elsewhere.
"""
import math

import numpy as np

from tests.olop_restatement import _first_max, kl_upper_bound, value_upper_init


def olop_stoch_plan(mode, transition, reward, terminal, s0, episodes, horizon, gamma, kl, thr, continuation, rng,
                    next_states=None, available=None, order=None, done_rule="source"):
    """One OLOP.plan from state ``s0`` on a dense (``mode`` "stochastic") or sparse model.  ``rng``: the planner's numpy
    Generator (advanced in place).  ``thr``: per-episode thresholds.  ``available`` [S, A] bool and ``order`` (listing order of
    the action ids) as ``get_available_actions`` lists them.  ``continuation``: "uniform" or anything else (action 0).
    Returns dict(plan, parent, action, depth, count, cum, mu, vu, done, state, env_steps, error); on an error ("key" /
    "range") the tree is the one at the raise."""
    transition = np.asarray(transition, np.float64)
    reward = np.asarray(reward, np.float64)
    term = np.zeros(reward.shape[0], bool) if terminal is None else np.asarray(terminal).astype(bool).reshape(-1)
    nxt = None if mode != "sparse" else np.asarray(next_states)
    n_actions, width = reward.shape[1], transition.shape[2]
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
        x = int(rng.integers(2 ** 30))                                         # olop.py:73
        clone = np.random.Generator(np.random.PCG64(np.random.SeedSequence(x)))
        node, path, s = 0, [0], int(s0)
        for h in range(int(horizon)):
            if not children[node]:
                acts = [a for a in order if available is None or available[s, a]]
                for a in acts:
                    children[node].append(new_node(node, a, depth[node] + 1, -1))
                act = int(rng.choice(acts)) if continuation == "uniform" else 0
            else:
                kids = children[node]
                act = action[kids[_first_max([vu[c] for c in kids])]]
            # the env's step (finite_mdp.py): one draw of the clone's generator, listed action or not
            r = float(reward[s, act])
            b = int(clone.choice(width, p=transition[s, act]))
            s_next = int(nxt[s, act, b]) if nxt is not None else b
            d = bool(term[s] if done_rule == "source" else term[s_next])
            s = s_next
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
                vu[n] = float(mu[n] + gamma * np.amax([vu[c] for c in children[n]]))
            else:
                vu[n] = mu[n]
    plan = []
    if error is None:
        node = 0
        while children[node]:
            kids = children[node]
            cnt = np.array([count[c] for c in kids])
            tops = np.flatnonzero(cnt == cnt.max())
            pick = kids[tops[_first_max([vu[kids[i]] for i in tops])]]
            plan.append(action[pick])
            node = pick
    return dict(plan=np.asarray(plan, np.int32), parent=np.asarray(parent, np.int32), action=np.asarray(action, np.int32),
                depth=np.asarray(depth, np.int32), count=np.asarray(count, np.int64), cum=np.asarray(cum, np.float64),
                mu=np.asarray(mu, np.float64), vu=np.asarray(vu, np.float64), done=np.asarray(done, np.uint8),
                state=np.asarray(state, np.int32), env_steps=env_steps, error=error)
