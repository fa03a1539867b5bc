#!/usr/bin/env python3
"""Golden vectors for GBOP: the UNMODIFIED reference
``rl_agents.agents.tree_search.graph_based_stochastic.StochasticGraphBasedPlannerAgent`` on deterministic, dense and sparse
finite-MDP tables.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_gbop.py      (build container only)

-> tests/golden/gbop.npz.  Per case: the MDP, the availability table and listing order of the environment, the config, the
seed; per ``plan()`` of the case the root, the generator record before and after, the plan (action and key) or the exception
with its message, the env steps and the planner's whole graph afterwards: the nodes in creation order (state, both bounds,
count, parents in order) and every chance record, packed by ``gbop_restatement.pack_listing`` (count, stored bounds, ``p_plus`` / ``p_minus``, the size of ``next_states``,
and the K transition children in DICT order: key -- a state, or -1 - i for ``placeholder_i`` --, count, cumulative reward,
``mu_ucb``, ``mu_lcb``).  Nothing of the reference is copied: inputs and its outputs only.

The adapters are those of make_golden_brue.py (``np.infty``, ``randint``, the 4-tuple ``step``, ``seed(x)``) and the ordered
parents of make_golden_gbopd.py: ``OrderedParentsDecisionNode``, a ``GraphDecisionNode`` subclass installed as
``StochasticGraphBasedPlanner.NODE_TYPE``, replaces ``parents`` by an insertion-ordered set and overrides nothing else.

MARGINS.  After every plan the test-side restatement (tests/gbop_restatement.py) replays it from the same generator record and
the script asserts that plan, generator record and the whole listing are equal BIT FOR BIT -- so the restatement's comparisons
are the reference's -- and takes from it every pair of numbers a comparison decides on: each value against the maximum in
``random_argmax``, ``delta`` against ``accuracy``, every pair ``max_expectation_under_constraint`` compares (f_star, theta_star,
isclose, the Newton steps, beta) and each entry of the cumulative ``p_minus`` against the double of ``choice``.  The script
REFUSES to write a file in which two compared numbers are neither equal nor more than 1e-9 apart; such a case gets another seed.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401
from make_golden import agent_factory, generators, np, put, put_mdp, rng_state  # noqa: E402

np.infty = np.inf
from make_golden_brue import StaleApiEnv, StaleGenerator  # noqa: E402
from make_golden_gape import MARGIN, load_agent_json  # noqa: E402
from make_golden_gbopd import InsertionOrderedSet, save_npz  # noqa: E402
from make_golden_olop_stoch import make_env  # noqa: E402

from rl_agents.agents.tree_search import graph_based_stochastic as ref  # noqa: E402

from rl_agents_amd import native  # noqa: E402
from tests import gbop_restatement as gb  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "gbop.npz"))
GBOP = "<class 'rl_agents.agents.tree_search.graph_based_stochastic.StochasticGraphBasedPlannerAgent'>"
ZERO = {"type": "kullback-leibler", "threshold": "0*np.log(time)", "transition_threshold": "0.1*np.log(time)"}


class OrderedParentsDecisionNode(ref.GraphDecisionNode):
    def __init__(self, planner, state, observation):
        super().__init__(planner, state, observation)
        self.parents = InsertionOrderedSet()


def install_adapter():
    ref.StochasticGraphBasedPlanner.NODE_TYPE = OrderedParentsDecisionNode


def key_of(k):
    return -1 - int(k[len("placeholder_"):]) if str(k).startswith("placeholder_") else int(k)


def graph_listing(planner, n_states, n_actions, K):
    nodes = list(planner.nodes.values())
    index = {id(n): i for i, n in enumerate(nodes)}
    n, A = len(nodes), n_actions
    out = dict(n_children=np.zeros(n, np.int32), action=np.full((n, A), -1, np.int32), c_count=np.zeros((n, A), np.int64),
               c_upper=np.zeros((n, A)), c_lower=np.zeros((n, A)), c_backed=np.full((n, A), -1, np.int32),
               k_state=np.zeros((n, A, K), np.int32), k_count=np.zeros((n, A, K), np.int64), k_cum=np.zeros((n, A, K)),
               k_mu_ucb=np.zeros((n, A, K)), k_mu_lcb=np.zeros((n, A, K)), p_plus=np.zeros((n, A, K)),
               p_minus=np.zeros((n, A, K)))
    ptr, idx = [0], []
    for i, node in enumerate(nodes):
        out["n_children"][i] = len(node.children)
        for k, (a, ch) in enumerate(node.children.items()):
            assert len(ch.children) == K
            out["action"][i, k], out["c_count"][i, k] = int(a), ch.count
            out["c_upper"][i, k], out["c_lower"][i, k] = float(ch.value_upper), float(ch.value_lower)
            if hasattr(ch, "next_states"):
                out["c_backed"][i, k] = sum(not str(x).startswith("placeholder_") for x in ch.next_states)
                out["p_plus"][i, k], out["p_minus"][i, k] = ch.p_plus, ch.p_minus
            for j, (key, d) in enumerate(ch.children.items()):
                out["k_state"][i, k, j], out["k_count"][i, k, j] = key_of(key), d.count
                out["k_cum"][i, k, j], out["k_mu_ucb"][i, k, j], out["k_mu_lcb"][i, k, j] = \
                    float(d.cumulative_reward), float(d.mu_ucb), float(d.mu_lcb)
        idx.extend(index[id(p)] for p in node.parents)
        ptr.append(len(idx))
    visits = np.zeros(n_states, np.int64)
    for k, v in planner.get_visits().items():
        visits[int(k)] = v
    out.update(state=np.asarray([int(x.observation) for x in nodes], np.int32),
               lower=np.asarray([float(x.value_lower) for x in nodes]), upper=np.asarray([float(x.value_upper) for x in nodes]),
               expanded=np.asarray([bool(x.children) for x in nodes], np.uint8),
               count=np.asarray([x.count for x in nodes], np.int64), parent_ptr=np.asarray(ptr, np.int32),
               parent_idx=np.asarray(idx, np.int32), visits=visits, n_observations=np.asarray(len(planner.observations)),
               root=np.asarray(index.get(id(planner.root), -1)))
    return out


def bits_equal(a, b):
    bad = []
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        same = x.shape == y.shape and np.array_equal(x, y)
        if same and x.dtype == np.float64:
            same = np.array_equal(x.view(np.uint64), np.asarray(y, np.float64).view(np.uint64))
        if not same:
            bad.append(k)
    return bad


def run_case(store, name, cfg, agent_cfg, seed, roots, available=None, order=None):
    """``roots``: the environment is put in each state in turn and ``agent.plan`` called on ONE planner object."""
    p = "gbop/" + name
    S, A = np.asarray(cfg["reward"]).shape
    put_mdp(store, p + "/mdp", cfg)
    put(store, p, dict(seed=seed, available=np.ones((S, A), bool) if available is None else np.asarray(available, bool),
                       order=np.arange(A) if order is None else np.asarray(order), masked=available is not None,
                       ordered=order is not None))
    if available is not None and not np.asarray(available).any(axis=1).all():
        # (the package's masked env refuses a state without an action at construction: the rows are cleared afterwards)
        env = make_env(cfg, roots[0], np.ones((S, A), bool), order)
        env.mdp.available = np.asarray(available, bool).copy()
    else:
        env = make_env(cfg, roots[0], available, order)
    agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=GBOP))
    agent.seed(seed)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    pc, ub = planner.config, planner.config["upper_bound"]
    K = int(pc["max_next_states_count"])
    put(store, p, dict(budget=pc["budget"], gamma=pc["gamma"], accuracy=pc["accuracy"], episodes=pc["episodes"],
                       horizon=pc["horizon"], sampling_timeout=pc["sampling_timeout"], max_next_states_count=K,
                       threshold=ub["threshold"], transition_threshold=ub["transition_threshold"],
                       horizon_given="horizon" in agent_cfg, n_plans=len(roots), roots=np.asarray(roots, np.int32)))
    mode = str(cfg["mode"])
    graph = gb.Graph(mode, cfg["transition"], cfg["reward"], pc["gamma"], K, cfg.get("next"), available, order)
    rthr = lambda c: gb.thresholds_by_count(ub["threshold"], pc["horizon"], A, pc["episodes"], c, c)[0]  # noqa: E731
    tthr = lambda c: gb.thresholds_by_count(ub["transition_threshold"], pc["horizon"], A, pc["episodes"], c, c)[0]  # noqa: E731
    pairs = []
    for i, s in enumerate(roots):
        env.mdp.state = int(s)
        q = "{}/plan{}".format(p, i)
        before = rng_state(planner.np_random)
        error, message, plan = "", "", []
        try:
            plan = agent.plan(int(s))
        except Exception as e:
            error, message = type(e).__name__, str(e)
        action = int(plan[0]) if plan else -1
        key = key_of(plan[1]) if len(plan) > 1 else 0
        lst = graph_listing(planner, S, A, K)
        put(store, q, dict(rng_before=before, rng_after=rng_state(planner.np_random), error=error, message=message,
                           plan_len=len(plan), action=action, key=key, env_steps=lst["n_observations"]))
        put(store, q + "/graph", gb.pack_listing(lst))
        # the restatement on the same generator record: bit for bit, then its comparisons are the reference's
        gen = np.random.Generator(np.random.PCG64(0))
        native.generator_set_state(gen, before)
        r_error, r_plan = "", []
        try:
            r_plan = graph.plan(int(s), pc["episodes"], pc["horizon"], pc["accuracy"], rthr, tthr, gen, pc["sampling_timeout"],
                                observe=lambda kind, a, b: pairs.append((float(a), float(b))))
        except (ValueError, TypeError) as e:
            r_error = type(e).__name__
            assert str(e) == message, (name, i, str(e), message)
        assert (r_error, [str(x) for x in r_plan]) == (error, [str(x) for x in plan]), (name, i, r_error, r_plan, error, plan)
        assert np.array_equal(native.rng_state_from_generator(gen), rng_state(planner.np_random)), (name, i)
        assert bits_equal(graph.listing(), lst) == [], (name, i, bits_equal(graph.listing(), lst))
        if error:
            put(store, p, dict(n_plans=i + 1))
            break
    return gb.smallest_margin(pairs), len(pairs)


def dense_of(sparse):
    """A dense [S, A, S] model with the rows of a sparse one (at most B successors a row)."""
    P, nxt = np.asarray(sparse["transition"], np.float64), np.asarray(sparse["next"])
    S, A, B = P.shape
    dense = np.zeros((S, A, S))
    for s in range(S):
        for a in range(A):
            for b in range(B):
                dense[s, a, nxt[s, a, b]] += P[s, a, b]
    return dict(mode="stochastic", transition=dense, reward=sparse["reward"], terminal=sparse["terminal"])


def cases():
    sailing = load_agent_json("SailingEnv/agents/gbop.json")
    assert sailing["max_next_states_count"] == 3 and sailing["upper_bound"]["threshold"] == "0*np.log(time)"
    evaluation = dict(gamma=0.8, upper_bound=ZERO, max_next_states_count=3, accuracy=5e-2)   # planners_evaluation.py:101-113
    det = generators.random_deterministic(12, 3, seed=201)
    det_term = generators.random_deterministic(10, 2, seed=202, terminal_rate=0.3)
    sparse2 = generators.random_sparse(10, 3, 2, seed=203)
    sparse3 = generators.random_sparse(9, 2, 3, seed=204, terminal_rate=0.2)
    dense3 = dense_of(generators.random_sparse(8, 3, 3, seed=205))
    sparse5 = generators.random_sparse(10, 5, 2, seed=206)
    avail5 = generators.random_available(10, 5, seed=207, rate=0.4)
    none_listed = np.ones((10, 3), bool)
    none_listed[np.asarray(sparse2["next"])[0, :, :].reshape(-1)[0]] = False
    by_count = dict(ZERO, transition_threshold="0.1*np.log(time) + 0.05*np.log(1 + count)")
    return [
        # name, mdp, agent config, seed, roots, available, listing order
        ("det_k1", det, dict(budget=60, gamma=0.8, upper_bound=ZERO), 0, [0, 0, 4], None, None),
        ("det_term_k2", det_term, dict(budget=60, gamma=0.7, upper_bound=ZERO, max_next_states_count=2), 1, [1], None, None),
        ("sparse_b2_k2", sparse2, dict(budget=80, gamma=0.8, upper_bound=ZERO, max_next_states_count=2), 2, [0, 0, 3], None, None),
        ("sparse_b2_k3", sparse2, dict(budget=80, gamma=0.8, upper_bound=ZERO, max_next_states_count=3), 3, [1], None, None),
        ("sparse_b3_sailing", sparse3, dict(sailing, budget=120), 4, [2], None, None),
        ("dense_b3_evaluation", dense3, dict(evaluation, budget=100), 5, [0, 1], None, None),
        ("masked_ordered_k2", sparse5, dict(budget=80, gamma=0.8, upper_bound=ZERO, max_next_states_count=2), 6, [3, 4],
         avail5, [1, 0, 4, 2, 3]),
        ("threshold_by_count", sparse2, dict(budget=80, gamma=0.9, accuracy=1e-3, upper_bound=by_count,
                                             max_next_states_count=3), 7, [2], None, None),
        ("horizon_given", sparse2, dict(horizon=3, episodes=12, gamma=0.8, upper_bound=ZERO, max_next_states_count=2), 8,
         [0], None, None),
        ("placeholders", sparse3, dict(budget=80, gamma=0.8, upper_bound=ZERO, max_next_states_count=2), 9, [0, 0], None, None),
        ("default_config", sparse2, dict(budget=60, max_next_states_count=2), 10, [0], None, None),
        ("no_listed_action", sparse2, dict(budget=60, gamma=0.8, upper_bound=ZERO, max_next_states_count=2), 11, [0, 0],
         none_listed, None),
    ]


def main():
    install_adapter()
    store, names, worst = {}, [], np.inf
    for name, cfg, agent_cfg, seed, roots, avail, order in cases():
        margin, n_pairs = run_case(store, name, cfg, agent_cfg, seed, roots, avail, order)
        last = int(store["gbop/{}/n_plans".format(name)]) - 1
        print("{:22s} {:10s} pairs {:7d} margin {:.3g}".format(name, str(store["gbop/{}/plan{}/error".format(name, last)]) or "ok",
                                                               n_pairs, margin), flush=True)
        assert margin > MARGIN, "case {}: two compared values are {} apart: choose another seed".format(name, margin)
        worst = min(worst, margin)
        names.append(name)
    store["gbop/names"] = np.asarray(names)
    store["gbop/margin"] = np.asarray(worst)
    get = lambda n, k: store["gbop/{}/{}".format(n, k)]  # noqa: E731
    last = lambda n: "plan{}".format(int(get(n, "n_plans")) - 1)  # noqa: E731
    # what the cases are there for
    assert str(get("placeholders", last("placeholders") + "/error")) == "ValueError"
    assert "placeholder" in str(get("placeholders", last("placeholders") + "/message"))
    assert str(get("default_config", "plan0/error")) == "TypeError" and int(get("default_config", "plan0/env_steps")) == 1
    assert str(get("default_config", "threshold")) == "1*np.log(time)"
    assert str(get("no_listed_action", last("no_listed_action") + "/error")) == "ValueError"
    for n in names:
        if n not in ("placeholders", "default_config", "no_listed_action"):
            assert all(not str(get(n, "plan{}/error".format(i))) for i in range(int(get(n, "n_plans")))), n
            assert all(int(get(n, "plan{}/plan_len".format(i))) == 2 for i in range(int(get(n, "n_plans")))), n
    assert {int(get(n, "max_next_states_count")) for n in names} >= {1, 2, 3}
    assert {str(get(n, "mdp/mode")) for n in names} == {"deterministic", "stochastic", "sparse"}
    assert (get("det_term_k2", last("det_term_k2") + "/graph/child_i")[0] < -1).any()         # a placeholder never assigned
    save_npz(OUT, store)
    size = os.path.getsize(OUT)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases, smallest margin", worst, size, "bytes")
    assert size <= os.path.getsize(os.path.join(os.path.dirname(OUT), "gape_stoch.npz")), size


if __name__ == "__main__":
    main()
