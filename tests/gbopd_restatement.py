"""GBOP-D (reference ``rl_agents/agents/tree_search/graph_based.py``) restated in plain Python for the tests: what a
``GraphBasedPlanner`` OBJECT computes over its lifetime on a deterministic finite-MDP table, operation for operation, on
arrays addressed by state -- the layout of ``mp_gbopd_export``.  It imports nothing of the reference; it is compared with the
reference's own outputs in tests/golden/gbopd.npz (tests/test_gbopd_host.py) and is what the device is compared with wherever
no golden exists (tests/test_gpu_gbopd.py).

The parents of a node are kept in INSERTION order (the order in which parents first expanded into it): the reference iterates
a set hashed by address there, this project fixes the order.
"""
import numpy as np


class Graph(object):
    """One planner's graph and lifetime counters.  ``available`` [S, A] bool and ``order`` (the environment's listing order,
    a permutation of the action ids) describe ``get_available_actions()``; without them every action in ascending order."""

    def __init__(self, transition, reward, gamma, available=None, order=None):
        self.T = np.asarray(transition, np.int64)
        self.R = np.asarray(reward, np.float64)
        self.S, self.A = self.R.shape
        self.gamma = gamma
        self.vmax = 1 / (1 - gamma)                         # graph_based.py:18 (ZeroDivisionError for gamma == 1)
        avail = np.ones((self.S, self.A), bool) if available is None else np.asarray(available, bool)
        order = list(range(self.A)) if order is None else [int(a) for a in order]
        self.listed = [[a for a in order if avail[s, a]] for s in range(self.S)]
        self.lower = np.zeros(self.S, np.float64)
        self.upper = np.zeros(self.S, np.float64)
        self.index = np.full(self.S, -1, np.int64)          # creation index, -1 = no node
        self.created = []                                   # states in creation order
        self.expanded = np.zeros(self.S, bool)
        self.parents = [[] for _ in range(self.S)]
        self.visits = np.zeros(self.S, np.int64)
        self.updates = np.zeros(self.S, np.int64)
        self.n_observations = 0
        self.root = -1
        self.pops = self.expansions = self.queue_peak = 0   # diagnostics (not part of the reference's state)

    # graph_based.py:110-116
    def get_node(self, s):
        if self.index[s] < 0:
            self.index[s] = len(self.created)
            self.created.append(s)
            self.lower[s], self.upper[s] = 0.0, self.vmax
        return s

    # graph_based.py:55-58, one field, in key order
    def backup(self, s, field):
        g, T, R = self.gamma, self.T, self.R
        return [float(R[s, a]) + g * float(field[T[s, a]]) for a in self.listed[s]]

    # graph_based.py:39-53
    def expand(self, s):
        for a in self.listed[s]:
            nxt = int(self.T[s, a])
            self.n_observations += 1                        # planner.step appends the observation (abstract.py:158-161)
            self.visits[nxt] += 1
            self.get_node(nxt)
            if s not in self.parents[nxt]:
                self.parents[nxt].append(s)
        self.expanded[s] = len(self.listed[s]) > 0
        self.expansions += 1

    # graph_based.py:66-78
    def partial_value_iteration(self, s, accuracy):
        queue, head = [s], 0
        while head < len(queue):
            self.updates[s] += 1                            # line 69 counts on the EXPANDED node
            self.queue_peak = max(self.queue_peak, len(queue) - head)
            node = queue[head]
            head += 1
            self.pops += 1
            delta = 0
            for field in (self.lower, self.upper):
                bound = max(self.backup(node, field))
                delta = max(delta, abs(float(field[node]) - bound))
                field[node] = bound
            if delta > accuracy:
                queue.extend(self.parents[node])

    # graph_based.py:96-108
    def run(self, root, accuracy, sampling_timeout, gen):
        node = root
        for _ in range(sampling_timeout):
            if not self.expanded[node]:
                self.expand(node)
                self.partial_value_iteration(node, accuracy)
                break
            q = np.asarray(self.backup(node, self.upper))                       # sampling_rule, :22-30
            pick = gen.choice(np.nonzero(q == np.amax(q))[0])                    # random_argmax (abstract.py:296-311)
            node = int(self.T[node, self.listed[node][pick]])
        else:
            self.n_observations += self.A                   # :108, n copies of the last node's observation
            self.visits[node] += self.A

    # graph_based.py:118-135
    def plan(self, root, budget, accuracy, sampling_timeout, gen):
        self.root = self.get_node(int(root))
        for _ in range(int(budget) // self.A):
            self.run(self.root, accuracy, sampling_timeout, gen)
        node, actions = self.root, []
        for _ in range(sampling_timeout):
            if not self.expanded[node]:
                break
            q = self.backup(node, self.lower)
            k = q.index(max(q))                             # selection_rule: Python max, the first maximum
            actions.append(self.listed[node][k])
            node = int(self.T[node, self.listed[node][k]])
        return actions

    def listing(self):
        """The graph in creation order, in the fields of tests/golden/gbopd.npz (``plan<i>/graph/...``)."""
        n, A = len(self.created), self.A
        child_action = np.full((n, A), -1, np.int32)
        child_node = np.full((n, A), -1, np.int32)
        child_reward = np.zeros((n, A), np.float64)
        n_children = np.zeros(n, np.int32)
        ptr, idx = [0], []
        for i, s in enumerate(self.created):
            if self.expanded[s]:
                for k, a in enumerate(self.listed[s]):
                    child_action[i, k], child_node[i, k], child_reward[i, k] = a, self.index[self.T[s, a]], self.R[s, a]
                n_children[i] = len(self.listed[s])
            idx.extend(int(self.index[p]) for p in self.parents[s])
            ptr.append(len(idx))
        st = np.asarray(self.created, np.int64)
        return dict(state=st.astype(np.int32), lower=self.lower[st].copy(), upper=self.upper[st].copy(),
                    expanded=self.expanded[st].astype(np.uint8), n_children=n_children, child_action=child_action,
                    child_node=child_node, child_reward=child_reward, parent_ptr=np.asarray(ptr, np.int32),
                    parent_idx=np.asarray(idx, np.int32), updates=self.updates.copy(), visits=self.visits.copy(),
                    n_observations=np.asarray(self.n_observations), root=np.asarray(int(self.index[self.root])))


GRAPH_KEYS = ("state", "lower", "upper", "expanded", "n_children", "child_action", "child_node", "child_reward", "parent_ptr",
              "parent_idx", "updates", "visits", "n_observations", "root")


def same_listing(a, b):
    """Field-by-field equality, doubles by bits (array_equal on finite values and the sign of zero)."""
    bad = []
    for k in GRAPH_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(k)
        elif x.dtype == np.float64 and not np.array_equal(x.view(np.uint64), np.asarray(y, np.float64).view(np.uint64)):
            bad.append(k + " (bits)")
    return bad
