#!/usr/bin/env python3
"""Golden vectors for MDP-GapE with several next states per chance node: the UNMODIFIED reference
``rl_agents.agents.tree_search.mdp_gape.MDPGapEAgent`` with ``max_next_states_count`` K >= 1 on deterministic, dense and
sparse finite-MDP tables.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_gape_stoch.py      (build container only)

-> tests/golden/gape_stoch.npz: per case the MDP, availability and listing order, the planner's config (K and the transition
threshold's string among it), the generator record before and after ``plan()``, the plan, ``episodes_run``, ``env_steps`` and
the whole tree (BFS listing over decision and chance nodes, children in the reference's DICT order: the placeholders left, then
the observed states by first observation; the key of ``placeholder_i`` is ``-1 - i``); or the exception the reference raised,
with its message, the step count and the generator record at the raise.  Nothing of the reference is copied: inputs and its
outputs only.

The adapters are those of make_golden_brue.py / make_golden_olop_stoch.py (``np.infty``, ``randint``, the 4-tuple ``step``,
``seed(x)`` -> the env's own ``seed(int(x))``).

MARGINS.  The observers of make_golden_gape.py ride along, and one more around ``max_expectation_under_constraint``: it calls
the reference's function, then the test-side restatement (tests/gape_stoch_restatement.py) on the same arguments, asserts that
the two results are equal bit for bit -- so the restatement's comparisons ARE the reference's -- and records every pair the
restatement compares: ``f_star`` against ``amax(f_p)``, ``theta_star`` against 0, each ``isclose`` difference against its
allowance, ``|x - x_next|`` against eps and ``x_next`` against ``a`` at every Newton iteration, ``beta`` against 0.  The script
REFUSES to write a file in which any recorded pair is neither equal nor more than 1e-9 apart; such a case gets another seed.
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
from make_golden_gape import GAPE, MARGIN, Observers, load_agent_json, ref  # noqa: E402
from make_golden_olop_stoch import make_env  # noqa: E402

from tests import gape_stoch_restatement as gs  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "gape_stoch.npz"))


class StochObservers(Observers):
    """The observers of the deterministic goldens, and the transition bound's comparisons."""

    def __init__(self):
        super(StochObservers, self).__init__()
        self.max_exp0 = ref.max_expectation_under_constraint
        self.newton, self.zero_mass = 0, 0

    def install(self):
        super(StochObservers, self).install()
        obs = self

        def max_exp(f, q, c, *args, **kwargs):
            p_ref = obs.max_exp0(f, q, c, *args, **kwargs)
            p, _, mask = gs.max_expectation(f, q, c, observe=lambda kind, a, b: obs.pairs.append((float(a), float(b))))
            assert np.array_equal(p, p_ref), (f, q, c, p, p_ref)
            obs.newton += bool(mask & gs.KT_NEWTON)
            obs.zero_mass += bool(mask & gs.KT_ZERO_MASS)
            return p_ref

        ref.max_expectation_under_constraint = max_exp

    def remove(self):
        super(StochObservers, self).remove()
        ref.max_expectation_under_constraint = self.max_exp0


def tree_listing(root):
    """BFS over both kinds of node, children in dict order.  A chance node's key is its action; a decision node's the observed
    state, or -1 - i for ``placeholder_i``."""
    chance = ref.ChanceNode

    def key(k):
        return -1 - int(k[len("placeholder_"):]) if isinstance(k, str) and k.startswith("placeholder_") else int(k)

    nodes, parents, keys = [root], [-1], [-1]
    i = 0
    while i < len(nodes):
        for k, c in nodes[i].children.items():
            nodes.append(c)
            parents.append(i)
            keys.append(key(k))
        i += 1
    dec = [not isinstance(n, chance) for n in nodes]
    return dict(parent=np.asarray(parents, np.int32), action=np.asarray(keys, np.int32),
                kind=np.asarray([0 if d else 1 for d in dec], np.uint8), depth=np.asarray([n.depth for n in nodes], np.int32),
                count=np.asarray([n.count for n in nodes], np.int64),
                cum=np.asarray([float(n.cumulative_reward) if d else 0.0 for n, d in zip(nodes, dec)]),
                mu_ucb=np.asarray([float(n.mu_ucb) if d else 0.0 for n, d in zip(nodes, dec)]),
                mu_lcb=np.asarray([float(n.mu_lcb) if d else 0.0 for n, d in zip(nodes, dec)]),
                vu=np.asarray([float(n.value_upper) for n in nodes]), vl=np.asarray([float(n.value_lower) for n in nodes]),
                done=np.asarray([bool(n.done) if d else False for n, d in zip(nodes, dec)], np.uint8))


def one_plan(store, p, cfg, s0, agent_cfg, seed, available=None, order=None):
    env = make_env(cfg, s0, available, order)
    shape = np.asarray(cfg["reward"]).shape
    put_mdp(store, p + "/mdp", cfg)
    put(store, p, dict(s0=s0, seed=seed, done_on_next=cfg.get("done_rule") == "next",
                       available=np.ones(shape, bool) if available is None else np.asarray(available, bool),
                       order=np.arange(shape[1]) if order is None else np.asarray(order)))
    agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=GAPE))
    agent.seed(seed)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    pc, ub = planner.config, planner.config["upper_bound"]
    put(store, p, dict(budget=pc["budget"], gamma=pc["gamma"], episodes=pc["episodes"], horizon=pc["horizon"],
                       accuracy=pc["accuracy"], confidence=pc["confidence"], continuation=pc["continuation_type"],
                       max_next_states_count=pc["max_next_states_count"], threshold=ub["threshold"],
                       transition_threshold=ub["transition_threshold"], rng_before=rng_state(planner.np_random)))
    obs = StochObservers()
    obs.install()
    try:
        plan = agent.plan(s0)
    except Exception as e:
        put(store, p, dict(error=type(e).__name__, message=str(e), rng_after=rng_state(planner.np_random),
                           env_steps=len(planner.observations)))
        return obs
    finally:
        obs.remove()
    assert planner.budget_used % pc["horizon"] == 0
    put(store, p, dict(error="", message="", plan=np.asarray(plan, np.int32), rng_after=rng_state(planner.np_random),
                       env_steps=len(planner.observations), episodes_run=planner.budget_used // pc["horizon"],
                       tie_draws=obs.tie_draws, margin=obs.smallest_margin(), newton=obs.newton, zero_mass=obs.zero_mass))
    put(store, p + "/tree", tree_listing(planner.root))
    return obs


def main():
    store, names = {}, []
    finite = load_agent_json("FiniteMDPEnv/agents/mdp-gape.json")
    assert finite["max_next_states_count"] == 2 and "transition_threshold" not in finite["upper_bound"]
    sparse2 = generators.random_sparse(12, 3, 2, seed=101)
    dense8 = generators.random_stochastic(8, 3, seed=102)
    det = generators.random_deterministic(20, 3, seed=103)
    sparse3 = generators.random_sparse(15, 3, 3, seed=104)
    sparse3_term = generators.random_sparse(15, 3, 2, seed=105, terminal_rate=0.25)
    dense_next = dict(generators.random_stochastic(6, 2, seed=106, terminal_rate=0.3), done_rule="next")
    sparse5 = generators.random_sparse(14, 5, 2, seed=107)
    avail5 = generators.random_available(14, 5, seed=108, rate=0.4)
    bad = generators.random_sparse(10, 3, 2, seed=109)
    bad["reward"] = np.asarray(bad["reward"]).copy()
    bad["reward"][4:, 2] = 1.5
    log_time = {"type": "kullback-leibler", "threshold": "1*np.log(time)"}
    by_count = dict(log_time, transition_threshold="0.1*np.log(time) + 0.05*np.log(1 + count)")
    cases = [
        # name, cfg, s0, agent config, seed, available, order
        ("finite_sparse_b2", sparse2, 0, finite, 0, None, None),
        ("finite_dense8_k8", dense8, 1, dict(finite, max_next_states_count=8), 1, None, None),
        ("finite_det_k2", det, 0, finite, 2, None, None),
        ("default_sparse_b3_k3", sparse3, 2, dict(budget=150, max_next_states_count=3), 3, None, None),
        ("det_k1", det, 3, dict(budget=120, gamma=0.8, accuracy=0.0, upper_bound=log_time), 4, None, None),
        ("placeholders", sparse3, 0, dict(budget=150, gamma=0.8, max_next_states_count=2, upper_bound=log_time), 5, None, None),
        ("terminal_source", sparse3_term, 1, dict(budget=120, gamma=0.8, accuracy=0.0, max_next_states_count=2,
                                                   upper_bound=log_time), 6, None, None),
        ("terminal_next", dense_next, 0, dict(budget=120, gamma=0.75, accuracy=0.0, max_next_states_count=6,
                                               upper_bound=log_time), 7, None, None),
        ("masked_ordered", sparse5, 3, dict(budget=150, gamma=0.8, accuracy=0.0, max_next_states_count=2, upper_bound=log_time),
         8, avail5, [1, 0, 4, 2, 3]),
        ("zeros", sparse2, 4, dict(budget=120, gamma=0.8, accuracy=0.0, max_next_states_count=2, continuation_type="zeros",
                                   upper_bound=log_time), 9, None, None),
        ("threshold_by_count", sparse2, 5, dict(budget=120, gamma=0.8, accuracy=0.0, max_next_states_count=3,
                                                upper_bound=by_count), 10, None, None),
        ("reward_range", bad, 0, dict(budget=100, gamma=0.8, max_next_states_count=2, upper_bound=log_time), 11, None, None),
        ("early_stop", sparse2, 1, dict(horizon=2, episodes=300, gamma=0.5, accuracy=0.9, max_next_states_count=2,
                                        upper_bound=log_time), 12, None, None),
    ]
    worst = np.inf
    for name, cfg, s0, agent_cfg, seed, avail, order in cases:
        obs = one_plan(store, "gape_stoch/" + name, cfg, s0, agent_cfg, seed, avail, order)
        margin = obs.smallest_margin()
        print("{:22s} {:12s} pairs {:7d} margin {:.3g} newton {} zero-mass {} tie draws {}".format(
            name, str(store["gape_stoch/" + name + "/error"]) or "ok", len(obs.pairs), margin, obs.newton, obs.zero_mass,
            obs.tie_draws))
        assert margin > MARGIN, "case {}: two compared values are {} apart: choose another seed".format(name, margin)
        worst = min(worst, margin)
        names.append(name)
    store["gape_stoch/names"] = np.asarray(names)
    store["gape_stoch/margin"] = np.asarray(worst)
    get = lambda n, k: store["gape_stoch/{}/{}".format(n, k)]  # noqa: E731
    # what the cases are there for
    assert str(get("placeholders", "error")) == "ValueError" and "placeholder" in str(get("placeholders", "message"))
    assert int(get("placeholders", "env_steps")) > int(get("placeholders", "horizon"))
    assert str(get("reward_range", "error")) == "ValueError" and int(get("reward_range", "env_steps")) > 1
    assert all(not str(get(n, "error")) for n in names if n not in ("placeholders", "reward_range"))
    assert int(get("early_stop", "episodes_run")) < int(get("early_stop", "episodes"))
    assert get("terminal_source", "tree/done").any() and get("terminal_next", "tree/done").any()
    for n in ("finite_sparse_b2", "finite_dense8_k8", "default_sparse_b3_k3"):
        assert int(get(n, "newton")) > 0 and int(get(n, "zero_mass")) > 0, n
    assert (get("finite_det_k2", "tree/action")[get("finite_det_k2", "tree/kind") == 0] < -1).any()   # a placeholder never assigned
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases, smallest margin", worst, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
