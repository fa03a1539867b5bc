"""GBOP, the graph-based optimistic planner for stochastic MDPs (reference
``rl_agents/agents/tree_search/graph_based_stochastic.py``) restated in plain Python + numpy for the tests: what a
``StochasticGraphBasedPlanner`` OBJECT computes over its lifetime on a deterministic, dense or sparse finite MDP, operation for
operation, on arrays addressed by state and by (state, action) -- the layout of ``mp_gbop_export``.  It imports nothing of the
reference; it is compared with the reference's own outputs in tests/golden/gbop.npz (tests/test_gbop_host.py) and is what the
device is compared with wherever no golden exists (tests/test_gpu_gbop.py).  The transition bound is
``tests.gape_stoch_restatement.max_expectation``, pinned on the reference bit for bit.

Known rewards only: a reward threshold other than 0 reaches the reference's mis-called ``kl_upper_bound`` (:79-82) and raises
TypeError; so it does here.  The parents of a node are kept in INSERTION order.

A chance node (s, a) holds K child SLOTS: slot j stands for ``placeholder_j`` until the j-th distinct next state is observed
and takes it (the lowest-numbered placeholder left, :207-219).  Python's dict moves an assigned placeholder to the end, so with
m states observed the reference's children are the slots m .. K-1, 0 .. m-1: :meth:`Graph.dict_order`.
"""
import numpy as np

from tests.gape_stoch_restatement import max_expectation

NO_PLACEHOLDER = ("No more placeholder nodes available, we observed more next states than "
                  "the 'max_next_states_count' config")
REWARD_THRESHOLD = "kl_upper_bound() got multiple values for argument 'threshold'"


def thresholds_by_count(expression, horizon, actions, episodes, first, last):
    """The threshold string of the config by count first .. last (:69-75, :200-205): ``time`` is the episodes of a plan."""
    time = episodes  # noqa: F841
    return np.asarray([float(eval(expression, {"np": np}, dict(horizon=horizon, actions=actions, count=count, time=time)))
                       for count in range(int(first), int(last) + 1)], np.float64)


class Graph(object):
    """One planner's graph, chance records and lifetime counters.  ``mode``: "deterministic" [S, A], "stochastic" [S, A, S] or
    "sparse" [S, A, B] with ``next_states``.  ``available`` [S, A] bool and ``order`` (the environment's listing order) describe
    ``get_available_actions()``; without them every action in ascending order."""

    def __init__(self, mode, transition, reward, gamma, max_next_states, next_states=None, available=None, order=None):
        self.mode = mode
        self.T = np.asarray(transition)
        self.R = np.asarray(reward, np.float64)
        self.nxt = None if next_states is None else np.asarray(next_states)
        self.S, self.A = self.R.shape
        self.K = K = int(max_next_states)
        self.gamma = gamma
        self.vmax = 1 / (1 - gamma)
        avail = np.ones((self.S, self.A), bool) if available is None else np.asarray(available, bool)
        order = list(range(self.A)) if order is None else [int(a) for a in order]
        self.listed = [[a for a in order if avail[s, a]] for s in range(self.S)]
        S, A = self.S, self.A
        self.lower, self.upper = np.zeros(S), np.zeros(S)
        self.index = np.full(S, -1, np.int64)
        self.created = []
        self.expanded = np.zeros(S, bool)
        self.parents = [[] for _ in range(S)]
        self.count = np.zeros(S, np.int64)                    # N(s) of planner.nodes[s]
        self.visits = np.zeros(S, np.int64)                   # get_visits(): the observations of planner.step
        self.n_observations = 0
        self.root = -1
        # chance records, by (state, action id)
        self.c_count = np.zeros((S, A), np.int64)
        self.c_upper = np.full((S, A), self.vmax)             # GraphNode.__init__: the stored bounds a count of 0 returns
        self.c_lower = np.zeros((S, A))
        self.c_assigned = np.zeros((S, A), np.int64)          # m: slots that stand for an observed state
        self.c_backed = np.full((S, A), -1, np.int64)         # m at the last backup (``next_states``), -1: never backed up
        self.k_state = np.tile(-1 - np.arange(K, dtype=np.int64), (S, A, 1))   # slot j: the state, -1 - j while a placeholder
        self.k_count = np.zeros((S, A, K), np.int64)
        self.k_cum = np.zeros((S, A, K))
        self.k_mu = np.ones((S, A, K))                        # mu_ucb
        self.k_mu_lcb = np.zeros((S, A, K))                   # mu_lcb: the same number once a reward was recorded
        self.p_plus = np.zeros((S, A, K))                     # in the dict order of the backup that wrote them
        self.p_minus = np.zeros((S, A, K))
        self.pops = self.queue_peak = 0                       # diagnostics: they change no result
        self.reset_diagnostics()

    def reset_diagnostics(self):
        """Per call of partial_value_iteration ``pvi_pushed`` (the initial queue plus every ``extend``) and ``pvi_peak`` (its
        longest length) are those of the LAST call; ``max_pushed`` / ``queue_peak`` their maxima and ``longest_update_queue`` the
        longest ``update_queue`` of a run since the graph was made or this was called; ``deepest_requeue`` the highest index
        at which a run found its state in ``update_queue`` already (-1: no run came back to a state)."""
        self.queue_peak = self.pvi_pushed = self.pvi_peak = self.max_pushed = self.longest_update_queue = 0
        self.deepest_requeue = -1

    def dict_order(self, s, a):
        m = int(self.c_assigned[s, a])
        return [(i + m) % self.K for i in range(self.K)]

    def get_node(self, s):
        if self.index[s] < 0:
            self.index[s] = len(self.created)
            self.created.append(s)
            self.lower[s], self.upper[s] = 0.0, self.vmax
        return s

    # GraphChanceNode.backup (:167-198)
    def chance_backup(self, s, a, upper, tthr, observe):
        n, K, g = int(self.c_count[s, a]), self.K, self.gamma
        self.c_backed[s, a] = self.c_assigned[s, a]
        if n == 0:
            self.p_plus[s, a] = self.p_minus[s, a] = np.ones((K,)) / K
            return float(self.c_upper[s, a] if upper else self.c_lower[s, a])
        slots = self.dict_order(s, a)
        p_hat = np.array([self.k_count[s, a, j] for j in slots]) / n
        threshold = tthr(n) / n
        nxt = np.zeros((K,))
        for i, j in enumerate(slots):
            st = int(self.k_state[s, a, j])
            if upper:
                v_n = float(self.upper[st]) if st >= 0 else 1 / (1 - g)
            else:
                v_n = float(self.lower[st]) if st >= 0 else 0
            nxt[i] = float(self.k_mu[s, a, j]) + g * v_n      # mu_ucb in BOTH bounds (:195)
        if upper:
            p = max_expectation(nxt, p_hat, threshold, observe=observe)[0]
            self.p_plus[s, a] = p
            self.c_upper[s, a] = p @ nxt
            return float(self.c_upper[s, a])
        p = max_expectation(-nxt, p_hat, threshold, observe=observe)[0]
        self.p_minus[s, a] = p
        self.c_lower[s, a] = p @ nxt
        return float(self.c_lower[s, a])

    def backup(self, s, upper, tthr, observe):
        return [self.chance_backup(s, a, upper, tthr, observe) for a in self.listed[s]]

    @staticmethod
    def random_argmax(values, gen, observe):
        if not values:
            raise ValueError("zero-size array to reduction operation maximum which has no identity")
        x = np.asarray(values)
        top = np.amax(x)
        for v in x:
            observe("argmax", top, v)
        return int(gen.choice(np.nonzero(x == top)[0]))

    # partial_value_iteration (:89-101)
    def partial_value_iteration(self, queue, accuracy, tthr, observe):
        head = 0
        self.pvi_pushed, self.pvi_peak = len(queue), 0
        while head < len(queue):
            self.pvi_peak = max(self.pvi_peak, len(queue) - head)
            node = queue[head]
            head += 1
            self.pops += 1
            delta = 0
            for upper, field in ((False, self.lower), (True, self.upper)):
                bound = np.amax(self.backup(node, upper, tthr, observe))
                delta = max(delta, abs(float(field[node]) - bound))
                field[node] = bound
            observe("delta", delta, accuracy)
            if delta > accuracy:
                queue.extend(self.parents[node])
                self.pvi_pushed += len(self.parents[node])
        self.queue_peak, self.max_pushed = max(self.queue_peak, self.pvi_peak), max(self.max_pushed, self.pvi_pushed)

    def step(self, s, a, clone):
        if self.mode == "deterministic":
            return int(self.T[s, a])
        b = int(clone.choice(self.T.shape[2], p=self.T[s, a]))
        return int(self.nxt[s, a, b]) if self.nxt is not None else b

    # run (:234-268)
    def run(self, root, horizon, accuracy, rthr, tthr, gen, observe):
        x = int(gen.integers(2 ** 30))
        clone = None if self.mode == "deterministic" else np.random.Generator(np.random.PCG64(np.random.SeedSequence(x)))
        s, update_queue = root, []
        for _ in range(horizon):
            self.get_node(s)
            self.expanded[s] = self.expanded[s] or bool(self.listed[s])           # expand (:103-105)
            a = self.listed[s][self.random_argmax(self.backup(s, True, tthr, observe), gen, observe)]
            s_next = self.step(s, a, clone)
            r = float(self.R[s, a])
            self.n_observations += 1
            self.visits[s_next] += 1
            # GraphChanceNode.get_child (:207-219)
            m = int(self.c_assigned[s, a])
            slot = [j for j in range(m) if self.k_state[s, a, j] == s_next]
            if slot:
                j = slot[0]
            else:
                if m == self.K:
                    raise ValueError(NO_PLACEHOLDER)
                j = m
                self.k_state[s, a, j] = s_next
                self.c_assigned[s, a] = m + 1
                self.get_node(s_next)
                if s not in self.parents[s_next]:
                    self.parents[s_next].append(s)
            self.count[s] += 1
            self.c_count[s, a] += 1
            self.k_count[s, a, j] += 1
            self.k_cum[s, a, j] += r
            if rthr(int(self.k_count[s, a, j])) != 0:
                raise TypeError(REWARD_THRESHOLD)
            self.k_mu[s, a, j] = self.k_mu_lcb[s, a, j] = self.k_cum[s, a, j] / self.k_count[s, a, j]
            if s not in update_queue:
                update_queue.append(s)
            else:
                self.deepest_requeue = max(self.deepest_requeue, update_queue.index(s))
            s = s_next
        self.longest_update_queue = max(self.longest_update_queue, len(update_queue))
        self.partial_value_iteration(list(reversed(update_queue)), accuracy, tthr, observe)

    def key_of(self, s, a, slot):
        st = int(self.k_state[s, a, slot])
        return str(st) if st >= 0 else "placeholder_{}".format(-1 - st)

    # plan (:332-337) and the inherited get_plan (graph_based.py:126-135)
    def plan(self, root, episodes, horizon, accuracy, rthr, tthr, gen, sampling_timeout=100, observe=None):
        """``rthr(count)`` / ``tthr(count)``: the reward / transition threshold by LIFETIME count.  Returns the reference's plan:
        [] , [action] or [action, key]; raises what the reference raises (the graph is then left as the reference leaves it)."""
        observe = observe or (lambda kind, a, b: None)
        self.root = self.get_node(int(root))
        for _ in range(int(episodes)):
            self.run(self.root, int(horizon), accuracy, rthr, tthr, gen, observe)
        plan, s = [], self.root
        if not self.expanded[s] or sampling_timeout < 1:
            return plan
        a = self.listed[s][self.random_argmax(self.backup(s, False, tthr, observe), gen, observe)]
        plan.append(a)
        if sampling_timeout < 2:
            return plan
        # GraphChanceNode.selection_rule (:152-156): Generator.choice(keys, p=p_minus)
        p = np.asarray(self.p_minus[s, a], np.float64)
        if np.isnan(p.sum()):
            raise ValueError("probabilities contain NaN")
        if (p < 0).any():
            raise ValueError("probabilities are not non-negative")
        if abs(float(np.sum(p)) - 1.0) > np.sqrt(np.finfo(np.float64).eps):
            raise ValueError("probabilities do not sum to 1")
        cdf = p.cumsum()
        cdf /= cdf[-1]
        u = gen.random()
        for c in cdf:
            observe("choice", c, u)
        i = int(cdf.searchsorted(u, side="right"))
        plan.append(self.key_of(s, a, self.dict_order(s, a)[i]))
        return plan

    def listing(self):
        """The graph in creation order with every chance record, in the fields of tests/golden/gbop.npz
        (``plan<i>/graph/...``).  Chance records [n, A, ...] by listing position; children [.., K] in dict order."""
        n, A, K = len(self.created), self.A, self.K
        st = np.asarray(self.created, np.int64)
        n_children = np.zeros(n, np.int32)
        action = np.full((n, A), -1, np.int32)
        c_count = np.zeros((n, A), np.int64)
        c_upper, c_lower = np.zeros((n, A)), np.zeros((n, A))
        c_backed = np.full((n, A), -1, np.int32)
        k_state = np.zeros((n, A, K), np.int32)
        k_count = np.zeros((n, A, K), np.int64)
        k_cum, k_mu_ucb, k_mu_lcb = np.zeros((n, A, K)), np.zeros((n, A, K)), np.zeros((n, A, K))
        p_plus, p_minus = np.zeros((n, A, K)), np.zeros((n, A, K))
        ptr, idx = [0], []
        for i, s in enumerate(self.created):
            if self.expanded[s]:
                n_children[i] = len(self.listed[s])
                for k, a in enumerate(self.listed[s]):
                    slots = self.dict_order(s, a)
                    action[i, k] = a
                    c_count[i, k], c_upper[i, k], c_lower[i, k] = self.c_count[s, a], self.c_upper[s, a], self.c_lower[s, a]
                    c_backed[i, k] = self.c_backed[s, a]
                    k_state[i, k] = self.k_state[s, a, slots]
                    k_count[i, k], k_cum[i, k] = self.k_count[s, a, slots], self.k_cum[s, a, slots]
                    k_mu_ucb[i, k] = self.k_mu[s, a, slots]
                    k_mu_lcb[i, k] = self.k_mu_lcb[s, a, slots]
                    if self.c_backed[s, a] >= 0:
                        p_plus[i, k], p_minus[i, k] = self.p_plus[s, a], self.p_minus[s, a]
            idx.extend(int(self.index[p]) for p in self.parents[s])
            ptr.append(len(idx))
        return dict(state=st.astype(np.int32), lower=self.lower[st].copy(), upper=self.upper[st].copy(),
                    expanded=self.expanded[st].astype(np.uint8), count=self.count[st].copy(), n_children=n_children,
                    action=action, c_count=c_count, c_upper=c_upper, c_lower=c_lower, c_backed=c_backed, k_state=k_state,
                    k_count=k_count, k_cum=k_cum, k_mu_ucb=k_mu_ucb, k_mu_lcb=k_mu_lcb, p_plus=p_plus, p_minus=p_minus,
                    parent_ptr=np.asarray(ptr, np.int32), parent_idx=np.asarray(idx, np.int32), visits=self.visits.copy(),
                    n_observations=np.asarray(self.n_observations), root=np.asarray(int(self.index[self.root])))


EXACT_KEYS = ("state", "expanded", "count", "n_children", "action", "c_count", "c_backed", "k_state", "k_count", "k_cum",
              "k_mu_ucb", "k_mu_lcb", "parent_ptr", "parent_idx", "visits", "n_observations", "root")
BOUND_KEYS = ("lower", "upper", "c_upper", "c_lower", "p_plus", "p_minus")


# the listing as the golden file stores it: the fields of one shape and kind stacked into one array (fewer zip members)
PACKED = {"nodes_i": ("state", "expanded", "count", "n_children"), "nodes_f": ("lower", "upper"),
          "chance_i": ("action", "c_count", "c_backed"), "chance_f": ("c_upper", "c_lower"), "child_i": ("k_state", "k_count"),
          "child_f": ("k_cum", "k_mu_ucb", "k_mu_lcb", "p_plus", "p_minus")}
DTYPES = dict(state=np.int32, expanded=np.uint8, n_children=np.int32, action=np.int32, c_backed=np.int32, k_state=np.int32)


def pack_listing(lst):
    out = {k: v for k, v in lst.items() if not any(k in names for names in PACKED.values())}
    for group, names in PACKED.items():
        out[group] = np.stack([np.asarray(lst[k], np.float64 if group.endswith("_f") else np.int64) for k in names])
    return out


def unpack_listing(arrays):
    out = {k: v for k, v in arrays.items() if k not in PACKED}
    for group, names in PACKED.items():
        for i, k in enumerate(names):
            out[k] = arrays[group][i].astype(DTYPES.get(k, arrays[group].dtype))
    return out


def compare_listing(a, b, tol):
    """The fields that differ: the discrete ones and the reward sums exactly, bounds and distributions within ``tol``."""
    bad = []
    for k in EXACT_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(k)
    for k in BOUND_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or not np.all(np.abs(x - y) <= tol):
            bad.append(k)
    return bad


def smallest_margin(pairs):
    d = [abs(a - b) for a, b in pairs if a != b and np.isfinite(a) and np.isfinite(b)]
    return min(d) if d else np.inf
