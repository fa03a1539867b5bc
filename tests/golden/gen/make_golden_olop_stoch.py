#!/usr/bin/env python3
"""Golden vectors for OLOP / KL-OLOP on STOCHASTIC finite MDPs: the UNMODIFIED reference
``rl_agents.agents.tree_search.olop.OLOPAgent`` on dense ([S, A, S]) and sparse ([S, A, B]) models of this package's
``FiniteMDPEnv`` family.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_olop_stoch.py      (build container only)

-> tests/golden/olop_stoch.npz: per case the MDP, the availability table and listing order, the planner's config, the
generator record before and after ``plan()``, the plan, the whole tree (BFS listing, children in creation order: parent,
action, depth, count, cum, mu, vu, done), ``env_steps``; or the exception the reference raised, with the step count and the
generator record at the raise.  Nothing of the reference is copied: inputs and its outputs only.

The adapters are those of make_golden_brue.py (``np.infty``, ``randint``, the 4-tuple ``step`` with done = terminated,
``seed(x)`` -> the env's own ``seed(int(x))``: the clone's generator of an episode is ``Generator(PCG64(SeedSequence(x)))``).
None changes what the reference computes.

Two OBSERVERS ride along, to prove from the reference's own run that the cases reach what they are here for.  Neither
changes a value: ``OLOPNode.update`` is wrapped by a function that looks at the node and then calls the original, and the
env adapter's ``step`` notes which actions the clone listed before it stepped.
* ``late_done``: some node's ``done`` was set at a visit later than its first (done is sticky per NODE, and only some
  realisations of a node reach a terminal state);
* ``reentered``: some node was entered in a state whose listed actions differ from the node's children (the children are
  fixed at the first expansion; the reference steps the selected child anyway).
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
from make_golden_olop import record_config, tree_listing  # noqa: E402
from rl_agents.agents.tree_search import olop as ref_olop  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "olop_stoch.npz"))
OLOP = "<class 'rl_agents.agents.tree_search.olop.OLOPAgent'>"

SEEN = dict(late_done=False, reentered=False, listed=None)


class ObservedEnv(StaleApiEnv):
    """StaleApiEnv that notes what the clone lists before a step (an observer: the step is the adapter's)."""

    def step(self, action):
        env = self.env
        SEEN["listed"] = list(env.get_available_actions()) if hasattr(env, "get_available_actions") \
            else list(range(env.action_space.n))
        return StaleApiEnv.step(self, action)


_update = ref_olop.OLOPNode.update


def observed_update(self, reward, done):
    """Looks, then calls the reference's own update."""
    if done and not self.done and self.count > 0:
        SEEN["late_done"] = True
    if self.parent is not None and list(self.parent.children.keys()) != SEEN["listed"]:
        SEEN["reentered"] = True
    return _update(self, reward, done)


ref_olop.OLOPNode.update = observed_update


def make_env(cfg, s0, available=None, order=None):
    c = {k: v for k, v in cfg.items() if k in ("mode", "transition", "reward", "terminal", "next")}
    c = {k: (np.asarray(v).tolist() if not isinstance(v, str) else v) for k, v in c.items()}
    c["state"], c["max_steps"] = int(s0), 0
    if cfg.get("done_rule"):
        c["done_rule"] = cfg["done_rule"]
    if order is not None:
        env = OrderedMaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist(), listing_order=list(order)))
    elif available is not None:
        env = MaskedFiniteMDPEnv(dict(c, available=np.asarray(available).astype(int).tolist()))
    else:
        env = FiniteMDPEnv(c)
    env.reset()
    return env


def one_plan(store, p, cfg, s0, agent_cfg, seed, available=None, order=None):
    SEEN.update(late_done=False, reentered=False, listed=None)
    env = make_env(cfg, s0, available, order)
    shape = np.asarray(cfg["reward"]).shape
    put_mdp(store, p + "/mdp", cfg)
    put(store, p, dict(s0=s0, seed=seed, done_on_next=cfg.get("done_rule") == "next", masked=available is not None,
                       available=np.ones(shape, bool) if available is None else np.asarray(available, bool),
                       order=np.arange(shape[1]) if order is None else np.asarray(order)))
    agent = agent_factory(ObservedEnv(env), dict(agent_cfg, __class__=OLOP))
    agent.seed(seed)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    record_config(store, p, planner.config)
    put(store, p, dict(rng_before=rng_state(planner.np_random)))
    try:
        plan = agent.plan(s0)
        error = ""
    except Exception as e:
        plan, error = [], type(e).__name__
    put(store, p, dict(error=error, plan=np.asarray(plan, np.int32), rng_after=rng_state(planner.np_random),
                       env_steps=len(planner.observations), late_done=SEEN["late_done"], reentered=SEEN["reentered"]))
    # (the tree at the raise is part of the record too: the nodes created and the updates made before it)
    put(store, p + "/tree", tree_listing(planner.root))
    return dict(error=error, env_steps=len(planner.observations), late_done=SEEN["late_done"], reentered=SEEN["reentered"],
                horizon=planner.config["horizon"], episodes=planner.config["episodes"])


def main():
    store, names, seen = {}, [], {}
    kl = {"type": "kullback-leibler", "time": "global", "threshold": "4*np.log(time)"}
    kl_local = dict(kl, time="local", threshold="2*np.log(time)")
    dense6 = generators.random_stochastic(6, 3, seed=81, terminal_rate=0.3)
    dense8 = dict(generators.random_stochastic(8, 2, seed=82, terminal_rate=0.3), done_rule="next")
    dense4 = generators.random_stochastic(4, 2, seed=83)
    sparse10 = generators.random_sparse(10, 3, 2, seed=84, terminal_rate=0.25)
    sparse12 = dict(generators.random_sparse(12, 2, 3, seed=85, terminal_rate=0.25), done_rule="next")
    sparse9 = generators.random_sparse(9, 3, 3, seed=86, terminal_rate=0.2)
    for cfg in (dense6, dense8, sparse10, sparse12, sparse9):
        assert np.asarray(cfg["terminal"]).any() and not np.asarray(cfg["terminal"]).all()
    avail6 = generators.random_available(6, 3, seed=87, rate=0.4)
    avail10 = generators.random_available(10, 3, seed=88, rate=0.4)
    avail9 = generators.random_available(9, 3, seed=89, rate=0.35)
    with0 = avail9.copy()
    with0[:, 0] = True                                   # "zeros" on a masked env that always lists action 0
    # "zeros" with action 0 unlisted: the first episode takes action 0 at every step and expands in the states it passes, so
    # action 0 is unlisted only in states that no walk of action 0 reaches within the horizon -- the raise comes in a later episode
    keyed, key_horizon = generators.random_sparse(12, 3, 2, seed=93), 3
    reach = {0}
    for _ in range(key_horizon - 1):
        reach |= {int(s) for r in reach for s in np.asarray(keyed["next"])[r, 0]}
    assert len(reach) < 12, reach
    no0 = np.ones((12, 3), bool)
    no0[[s for s in range(12) if s not in reach], 0] = False
    bad = generators.random_stochastic(6, 3, seed=91)
    bad["reward"] = np.asarray(bad["reward"]).copy()
    bad["reward"][3:, 2] = 1.25                          # out of [0, 1] in some rows only: the raise comes mid-plan
    edge = generators.random_sparse(8, 3, 3, seed=92, terminal_rate=0.2)
    edge["reward"] = np.where(np.asarray(edge["reward"]) < 0.3, 0.0, np.where(np.asarray(edge["reward"]) > 0.7, 1.0,
                                                                              np.asarray(edge["reward"])))
    cases = [
        # name, cfg, s0, agent config, seed, available, order
        ("dense_kl_global_uniform", dense6, 0, dict(horizon=4, episodes=40, gamma=0.8, continuation_type="uniform", upper_bound=kl),
         0, None, None),
        ("dense_next_kl_local_zeros", dense8, 1, dict(horizon=5, episodes=50, gamma=0.85, upper_bound=kl_local), 1, None, None),
        ("dense_budget_kl", dense4, 2, dict(budget=60, gamma=0.8, upper_bound=kl), 2, None, None),
        ("sparse_b2_kl_global_zeros", sparse10, 0, dict(horizon=4, episodes=60, gamma=0.8, upper_bound=kl), 3, None, None),
        ("sparse_b3_next_kl_local_uniform", sparse12, 3, dict(horizon=6, episodes=45, gamma=0.9, continuation_type="uniform",
                                                                upper_bound=kl_local), 4, None, None),
        ("sparse_b3_kl_01_rewards", edge, 1, dict(horizon=3, episodes=60, gamma=0.7, continuation_type="uniform", upper_bound=kl),
         5, None, None),
        ("dense_default_hoeffding_uniform", dense6, 2, dict(horizon=3, episodes=30, gamma=0.8, continuation_type="uniform"), 6, None, None),
        ("sparse_laplace_zeros", sparse9, 0, dict(horizon=4, episodes=30, gamma=0.8, upper_bound=dict(kl, type="laplace")), 7, None, None),
        ("masked_dense_kl_uniform", dense6, 1, dict(horizon=4, episodes=50, gamma=0.8, continuation_type="uniform", upper_bound=kl),
         8, avail6, None),
        ("masked_sparse_kl_local_uniform", sparse10, 2, dict(horizon=5, episodes=50, gamma=0.85, continuation_type="uniform",
                                                              upper_bound=kl_local), 9, avail10, None),
        ("ordered_sparse_kl_uniform", sparse9, 4, dict(horizon=4, episodes=50, gamma=0.8, continuation_type="uniform", upper_bound=kl),
         10, avail9, [2, 0, 1]),
        ("ordered_sparse_kl_zeros", sparse9, 5, dict(horizon=4, episodes=40, gamma=0.8, upper_bound=kl), 11, with0, [1, 2, 0]),
        ("masked_zeros_keyerror", keyed, 0, dict(horizon=key_horizon, episodes=40, gamma=0.8, upper_bound=kl), 12, no0, None),
        ("reward_range", bad, 0, dict(horizon=3, episodes=40, gamma=0.8, continuation_type="uniform", upper_bound=kl), 13, None, None),
    ]
    for name, cfg, s0, agent_cfg, seed, avail, order in cases:
        seen[name] = one_plan(store, "olop_stoch/" + name, cfg, s0, agent_cfg, seed, avail, order)
        assert seen[name]["horizon"] <= 6 and seen[name]["episodes"] <= 60, name
        names.append(name)
        print(name, seen[name])
    store["olop_stoch/names"] = np.asarray(names)

    # what the cases are here for, from the reference's own run
    assert any(v["late_done"] for v in seen.values()), "no node's done was set after its first visit"
    assert any(v["late_done"] for k, v in seen.items() if k.startswith("dense_next") or k.startswith("sparse_b3_next")), \
        "no late done under the 'next' rule"
    for name in ("masked_dense_kl_uniform", "masked_sparse_kl_local_uniform", "ordered_sparse_kl_uniform"):
        assert seen[name]["reentered"] and not seen[name]["error"], name
    for name, v in seen.items():
        if not name.startswith(("masked", "ordered")):
            assert not v["reentered"], name
    key = seen["masked_zeros_keyerror"]
    assert key["error"] == "KeyError" and key["env_steps"] > key["horizon"], key            # raised in a later episode
    rng = seen["reward_range"]
    assert rng["error"] == "ValueError" and rng["env_steps"] > rng["horizon"], rng
    assert all(not v["error"] for k, v in seen.items() if k not in ("masked_zeros_keyerror", "reward_range")), seen
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays,", len(names), "cases")


if __name__ == "__main__":
    main()
