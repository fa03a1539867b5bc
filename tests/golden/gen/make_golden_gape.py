#!/usr/bin/env python3
"""Golden vectors for MDP-GapE: the UNMODIFIED reference ``rl_agents.agents.tree_search.mdp_gape.MDPGapEAgent`` on
deterministic finite-MDP tables with ``max_next_states_count: 1``.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_gape.py      (build container only)

-> tests/golden/gape.npz: per case the MDP, availability and listing order, the planner's config, the generator record
before and after ``plan()``, the plan, ``episodes_run`` (``budget_used / horizon``), ``env_steps`` and the whole tree (BFS
listing over decision and chance nodes, children in creation order); or the exception the reference raised, with the step
count and the generator record at the raise.  Nothing of the reference is copied: inputs and its outputs only.

The adapters are those of make_golden_olop.py (``np.infty``, ``randint``, the 4-tuple ``step``, a no-op ``seed``).

MARGINS.  A plan hangs on comparisons of bounds, and the device's KL bound agrees with numpy's only to 1e-12.  Observers that
call the reference's own methods record every pair of numbers it compares -- the gaps under ``min``, the rest's ``value_upper``
under ``max``, the two widths, every ``random_argmax`` list against its maximum, the stopping test -- and the script REFUSES to
write a file in which any pair is neither exactly equal nor more than 1e-9 apart: a value sums at most 1 / (1 - gamma) <= 20
terms of 1e-12, so 1e-9 leaves a factor 50.  A case that breaks the condition is given another seed.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import agent_factory, generators, np, put, put_mdp, rng_state  # noqa: E402
from make_golden_olop import StaleApiEnv, StaleGenerator, make_env  # noqa: E402

from rl_agents.agents.tree_search import mdp_gape as ref  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "gape.npz"))
GAPE = "<class 'rl_agents.agents.tree_search.mdp_gape.MDPGapEAgent'>"
REF_CFG = os.path.join(mg.REF, "scripts", "configs")
MARGIN = 1e-9


class Observers(object):
    """Wraps the reference's comparing methods; every wrapper calls the original and returns what it returned."""

    def __init__(self):
        self.pairs, self.unlisted, self.tie_draws = [], 0, 0
        self.bai0, self.argmax0, self.get_child0, self.run0 = (ref.DecisionNode.best_arm_identification_selection,
                                                               ref.DecisionNode.random_argmax, ref.DecisionNode.get_child,
                                                               ref.MDPGapE.run)

    def running(self, values, sign):
        """The pairs a first-minimum (sign -1) / first-maximum (sign +1) scan compares."""
        cur = values[0]
        for v in values[1:]:
            self.pairs.append((float(cur), float(v)))
            if sign * (v - cur) > 0:
                cur = v

    def install(self):
        obs = self

        def bai(node):
            selected, best, challenger = obs.bai0(node)
            kids = list(node.children.values())
            obs.running([c.gap for c in kids], -1)
            obs.running([c.value_upper for c in kids if c is not best], +1)
            obs.running([n.value_upper - n.value_lower for n in (best, challenger)], +1)
            return selected, best, challenger

        def random_argmax(node, x):
            top = np.amax(x)
            obs.pairs.extend((float(top), float(v)) for v in x)
            obs.tie_draws += int(np.sum(np.asarray(x) == top) > 1)
            return obs.argmax0(node, x)

        def get_child(node, action, state):
            chance, taken = obs.get_child0(node, action, state)
            obs.unlisted += int(taken != action)
            return chance, taken

        def run(planner, state):
            best, challenger = obs.run0(planner, state)
            obs.pairs.append((float(challenger.value_upper - best.value_lower), float(planner.config["accuracy"])))
            return best, challenger

        ref.DecisionNode.best_arm_identification_selection = bai
        ref.DecisionNode.random_argmax = random_argmax
        ref.DecisionNode.get_child = get_child
        ref.MDPGapE.run = run

    def remove(self):
        ref.DecisionNode.best_arm_identification_selection = self.bai0
        ref.DecisionNode.random_argmax = self.argmax0
        ref.DecisionNode.get_child = self.get_child0
        ref.MDPGapE.run = self.run0

    def smallest_margin(self):
        d = [abs(a - b) for a, b in self.pairs if a != b and np.isfinite(a) and np.isfinite(b)]
        return min(d) if d else np.inf


def tree_listing(root):
    """BFS over both kinds of node, children in dict (= creation) order.  A chance node's key is its action, a decision
    node's the observed state."""
    chance = ref.ChanceNode
    nodes, parents, keys = [root], [-1], [-1]
    i = 0
    while i < len(nodes):
        for k, c in nodes[i].children.items():
            nodes.append(c)
            parents.append(i)
            keys.append(int(k))
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


def load_agent_json(rel):
    import json
    with open(os.path.join(REF_CFG, rel)) as f:
        cfg = json.load(f)
    return {k: v for k, v in cfg.items() if k not in ("__class__", "env_preprocessors")}


def one_plan(store, p, cfg, s0, agent_cfg, seed, available=None, order=None):
    env = make_env(cfg, s0, available, order, 0)
    n_actions = np.asarray(cfg["reward"]).shape[1]
    put_mdp(store, p + "/mdp", cfg)
    put(store, p, dict(s0=s0, seed=seed, done_on_next=cfg.get("done_rule") == "next",
                       available=np.ones(np.asarray(cfg["reward"]).shape, bool) if available is None else available,
                       order=np.arange(n_actions) if order is None else np.asarray(order)))
    agent = agent_factory(StaleApiEnv(env), dict(agent_cfg, __class__=GAPE))
    agent.seed(seed)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    pc, ub = planner.config, planner.config["upper_bound"]
    put(store, p, dict(budget=pc["budget"], gamma=pc["gamma"], episodes=pc["episodes"], horizon=pc["horizon"],
                       accuracy=pc["accuracy"], confidence=pc["confidence"], continuation=pc["continuation_type"],
                       horizon_from_accuracy=pc["horizon_from_accuracy"], threshold=ub["threshold"],
                       horizon_given="horizon" in agent_cfg, rng_before=rng_state(planner.np_random)))
    obs = Observers()
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
                       unlisted=obs.unlisted, tie_draws=obs.tie_draws, margin=obs.smallest_margin()))
    put(store, p + "/tree", tree_listing(planner.root))
    return obs


def main():
    store, names = {}, []
    rnd = generators.random_deterministic(30, 3, seed=81)
    small = generators.random_deterministic(12, 3, seed=82)
    rnd5 = generators.random_deterministic(50, 5, seed=83, terminal_rate=0.1)
    avail5 = generators.random_available(50, 5, seed=84, rate=0.4)
    nxt = dict(generators.random_deterministic(30, 4, seed=85, terminal_rate=0.2), done_rule="next")
    wide = generators.random_deterministic(40, 70, seed=86)
    bad = generators.random_deterministic(20, 3, seed=87)
    bad["reward"] = bad["reward"].copy()
    bad["reward"][:, 2] = 1.5
    one = generators.random_deterministic(10, 1, seed=88)
    highway = load_agent_json("HighwayEnv/agents/MDPGapEAgent/baseline.json")
    log_time = {"type": "kullback-leibler", "threshold": "1*np.log(time)"}
    cases = [
        # name, cfg, s0, agent config, seed, available, order
        ("default_300", rnd, 0, dict(budget=300), 0, None, None),
        ("zeros", rnd, 3, dict(budget=200, continuation_type="zeros"), 1, None, None),
        ("masked_uniform", rnd5, 3, dict(budget=250), 2, avail5, None),
        ("masked_zeros", rnd5, 7, dict(budget=250, continuation_type="zeros"), 3, avail5, None),
        ("ordered", rnd5, 3, dict(budget=250), 4, avail5, [1, 0, 4, 2, 3]),
        ("done_next", nxt, 4, dict(budget=200, gamma=0.75), 5, None, None),
        ("given_horizon", rnd, 6, dict(horizon=4, episodes=20, gamma=0.9), 6, None, None),
        ("horizon_from_accuracy", rnd, 2, dict(budget=300, accuracy=0.5, horizon_from_accuracy=True), 7, None, None),
        ("highway_baseline", rnd5, 1, highway, 8, None, None),
        ("early_stop", small, 0, dict(horizon=2, episodes=400, gamma=0.5, accuracy=0.6, upper_bound=log_time), 9, None, None),
        ("full_run", small, 5, dict(horizon=3, episodes=30, gamma=0.8, accuracy=0.0), 10, None, None),
        ("wide_70", wide, 0, dict(horizon=3, episodes=150, gamma=0.8, upper_bound=log_time), 11, None, None),
        ("horizon_40", rnd, 1, dict(horizon=40, episodes=8, gamma=0.9, upper_bound=log_time), 12, None, None),
        ("reward_range", bad, 0, dict(budget=100), 13, None, None),
        ("one_action", one, 0, dict(budget=50), 14, None, None),
        ("confidence_one", rnd, 0, dict(budget=100, confidence=1.0), 15, None, None),
    ]
    worst = np.inf
    for name, cfg, s0, agent_cfg, seed, avail, order in cases:
        obs = one_plan(store, "gape/" + name, cfg, s0, agent_cfg, seed, avail, order)
        margin = obs.smallest_margin()
        print("{:24s} {:18s} pairs {:7d} margin {:.3g} unlisted {} tie draws {}".format(
            name, str(store["gape/" + name + "/error"]) or "ok", len(obs.pairs), margin, obs.unlisted, obs.tie_draws))
        assert margin > MARGIN, "case {}: two compared values are {} apart: choose another seed".format(name, margin)
        worst = min(worst, margin)
        names.append(name)
    store["gape/names"] = np.asarray(names)
    store["gape/margin"] = np.asarray(worst)
    get = lambda n, k: store["gape/{}/{}".format(n, k)]  # noqa: E731
    # what the cases are there for
    assert int(get("masked_uniform", "unlisted")) > 0 and int(get("masked_zeros", "unlisted")) > 0
    assert int(get("early_stop", "episodes_run")) < int(get("early_stop", "episodes"))
    assert int(get("full_run", "episodes_run")) == int(get("full_run", "episodes")) + 2
    assert [str(get(n, "error")) for n in ("reward_range", "one_action", "confidence_one")] == ["ValueError", "ValueError",
                                                                                                "ZeroDivisionError"]
    assert get("done_next", "tree/done").any()
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases, smallest margin", worst, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
