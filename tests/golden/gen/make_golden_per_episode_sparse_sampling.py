#!/usr/bin/env python3
"""Golden vectors for Sparse Sampling on a BATCH OF EPISODES WITH THEIR OWN, PER-STEP-CHANGING TABLES
(tests/golden/per_episode_sparse_sampling.npz).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_per_episode_sparse_sampling.py      (build container only)

As make_golden_per_episode.py: E episodes each own a highway-shaped (3, 4, 10) table that is REPLACED before every step (as a
re-extraction with to_finite_mdp() would), and the UNMODIFIED reference ``SparseSamplingAgent`` -- one object per episode,
seeded 100 + e, ``horizon 3, C 2, gamma 0.8`` -- is driven step by step through the stale-API adapters of
make_golden_sparse_sampling.py (``np.infty``, ``randint``, the 4-tuple ``step``, ``seed``), none of which changes what it
computes.  The tables, start states and seeds are the ones per_episode.npz holds (the same generator calls); the fixture stores
them again so that it stands alone; one more episode (tables and seed by the same rule) starts in a state from which the
reference's own actions end it before the last step.  Per step: the plan, the generator record before and after it, the value
of the root's chosen chance child and how many of the root's chance children hold the maximum (two or more: ``random_argmax``
drew among them, abstract.py:296-311).  Data only: inputs and outputs.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_sparse_sampling import SS, StaleApiEnv, StaleGenerator  # noqa: E402  (aliases np.infty before the reference is imported)
from make_golden import agent_factory, np, rng_state  # noqa: E402
from make_golden_per_episode import E, L, T_STEPS, TT, V, install, table  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "per_episode_sparse_sampling.npz"))
CONFIG = {"horizon": 3, "C": 2, "gamma": 0.8}


def run_episode(e, start, tabs):
    """One reference agent, seeded 100 + e, on episode e's tables from state ``start`` -> (arrays, steps, most root ties)."""
    store, most_ties = {}, 0
    cfg0 = dict(tabs[0])
    cfg0.pop("original_shape", None)
    cfg0["state"] = int(start)
    env = FiniteMDPEnv(cfg0)
    env.reset()
    agent = agent_factory(StaleApiEnv(env), dict(CONFIG, __class__=SS))
    agent.seed(100 + e)
    planner = agent.planner
    planner.np_random = StaleGenerator(planner.np_random.bit_generator)
    store["ss/e{}/rng_before".format(e)] = rng_state(planner.np_random)
    pc = planner.config
    for k in ("gamma", "horizon", "C"):
        store["ss/{}".format(k)] = np.asarray(pc[k])
    states, n_steps = [], 0
    for t in range(T_STEPS):
        install(env, tabs[t])
        s = env.mdp.state
        states.append(s)
        p = "ss/e{}/t{}".format(e, t)
        planner.np_random = StaleGenerator(planner.np_random.bit_generator)
        store[p + "/rng_before"] = rng_state(planner.np_random)
        plan = [int(a) for a in agent.plan(s)]
        values = [float(c.value) for c in planner.root.children.values()]
        ties = int(sum(v == max(values) for v in values))
        most_ties = max(most_ties, ties)
        store[p + "/plan"] = np.asarray(plan, np.int32)
        store[p + "/rng_after"] = rng_state(planner.np_random)
        store[p + "/root_value"] = np.asarray(float(planner.root.children[plan[0]].value))
        store[p + "/root_ties"] = np.asarray(ties)
        store[p + "/env_steps_total"] = np.asarray(len(planner.observations))
        n_steps += 1
        _, _, term, trunc, _ = env.step(plan[0])
        if term or trunc:
            break
    store["ss/e{}/states".format(e)] = np.asarray(states, np.int64)
    store["ss/e{}/n_steps".format(e)] = np.asarray(n_steps)
    return store, n_steps, most_ties


def main():
    store = {}
    tabs = [[table(e, t) for t in range(T_STEPS)] for e in range(E + 1)]
    s0 = [((e % V) * L + (e % L)) * TT for e in range(E)]             # time slice 0 of some (speed, lane)
    most_ties, lengths = 0, []
    for e in range(E):
        arrays, n_steps, ties = run_episode(e, s0[e], tabs[e])
        store.update(arrays)
        most_ties = max(most_ties, ties)
        lengths.append(n_steps)
    # The reference's Sparse Sampling agents steer the E episodes of per_episode.npz clear of every collision for T_STEPS steps.
    # One more episode, tables and seed by the same rule, starts in the first state from which its agent's own actions end it
    # early: the batch has to drop it from the live set.
    for start in range(V * L * TT):
        arrays, n_steps, ties = run_episode(E, start, tabs[E])
        if n_steps < T_STEPS:
            break
    assert n_steps < T_STEPS, "no start state ends episode {} early".format(E)
    store.update(arrays)
    s0.append(start)
    lengths.append(n_steps)
    most_ties = max(most_ties, ties)
    store["transition"] = np.stack([np.stack([c["transition"] for c in row]) for row in tabs]).astype(np.int64)   # [E + 1,T,S,A]
    store["reward"] = np.stack([np.stack([c["reward"] for c in row]) for row in tabs]).astype(np.float64)
    store["terminal"] = np.stack([np.stack([c["terminal"] for c in row]) for row in tabs]).astype(bool)
    store["s0"] = np.asarray(s0, dtype=np.int64)
    # the tie draw of random_argmax must be in the fixture
    assert most_ties >= 2, "no recorded plan has two maximal chance children at its root"
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays", os.path.getsize(OUT), "bytes; most maximal root children:", most_ties, "steps:", lengths,
          "start states:", s0)


if __name__ == "__main__":
    main()
