#!/usr/bin/env python3
"""Golden vectors for the discrete robust planner on a BATCH OF EPISODES THAT EACH OWN A SET OF M MODELS, REPLACED BEFORE EVERY
STEP (tests/golden/per_episode_robust.npz).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_per_episode_robust.py      (build container only)

``DiscreteRobustPlannerAgent.plan`` builds its models again before every plan (agents/robust/robust.py:68-71): on an environment
whose table is extracted again at every step, each episode has its own M hypothesis tables at each step.  As
make_golden_per_episode.py: E episodes each own a highway-shaped (3, 4, 10) table that is REPLACED before every step -- the very
tables per_episode.npz holds -- and hypothesis m > 0 of a step is ``generators.rewire`` of that step's table with its own seed.
The UNMODIFIED reference ``DiscreteRobustPlanner`` -- one planner object per episode, seeded once (100 + e), its generator
continuing from step to step -- plans on the ``JointEnv5`` stand-in of make_golden_robust.py (the reference's JointEnv with the
5-tuple step, nothing more), after ``step_by_reset()`` as AbstractTreeSearchAgent.plan does first.  The true environment follows
table 0.  Per step: the plan, the root's bounds (min over the models), the generator record after it and the planner's total of
env steps.  Data only: inputs and outputs.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import make_env, np, rng_state  # noqa: E402
from make_golden_per_episode import E, L, T_STEPS, TT, V, install, table  # noqa: E402
from make_golden_robust import DiscreteRobustPlanner, JointEnv5  # noqa: E402

from rl_agents_amd.envs import generators  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "per_episode_robust.npz"))
CONFIGS = dict(
    m2=(2, dict(budget=150, gamma=0.8)),
    m3=(3, dict(budget=100, gamma=0.9, terminal_reward=0.5)),
)
REWIRE = (None, 0.15, 0.3)


def hypotheses(e, t, m_models):
    base = table(e, t)
    out = [base]
    for m in range(1, m_models):
        out.append(generators.rewire(base, REWIRE[m], seed=7000 + 100 * e + 10 * t + m))
    return out


def main():
    store = {}
    s0 = np.array([((e % V) * L + (e % L)) * TT for e in range(E)], dtype=np.int64)     # as per_episode.npz
    store["s0"] = s0
    for name, (m_models, pcfg) in CONFIGS.items():
        tabs = [[hypotheses(e, t, m_models) for t in range(T_STEPS)] for e in range(E)]
        store[name + "/transition"] = np.asarray([[[c["transition"] for c in step] for step in row] for row in tabs], np.int64)  # [E,T,M,S,A]
        store[name + "/reward"] = np.asarray([[[c["reward"] for c in step] for step in row] for row in tabs], np.float64)
        store[name + "/terminal"] = np.asarray([[[c["terminal"] for c in step] for step in row] for row in tabs]).astype(bool)
        store[name + "/n_models"] = np.asarray(m_models)
        for k in ("budget", "gamma"):
            store["{}/{}".format(name, k)] = np.asarray(pcfg[k])
        store[name + "/terminal_reward"] = np.asarray(pcfg.get("terminal_reward", 0))
        for e in range(E):
            env = make_env(tabs[e][0][0], state=int(s0[e]))        # the true environment: table 0 of every step
            joint = JointEnv5([make_env(c, state=int(s0[e])) for c in tabs[e][0]])
            planner = DiscreteRobustPlanner(joint, dict(dict(terminal_reward=0), **pcfg))
            planner.seed(100 + e)
            store["{}/e{}/rng_before".format(name, e)] = rng_state(planner.np_random)
            states, n_steps = [], 0
            for t in range(T_STEPS):
                install(env, tabs[e][t][0])
                s = int(env.mdp.state)
                states.append(s)
                # robust.py:69-70: the M models, built again from the true environment as it is now
                joint = JointEnv5([make_env(c, state=s, steps=env.steps) for c in tabs[e][t]])
                planner.step_by_reset()
                plan = [int(a) for a in planner.plan(joint, s)]
                assert all(x.mdp.state == s for x in joint.joint_state)          # the models were never stepped
                p = "{}/e{}/t{}".format(name, e, t)
                store[p + "/plan"] = np.asarray(plan, np.int32)
                store[p + "/root_lower"] = np.asarray(float(np.min(planner.root.value_lower)))
                store[p + "/root_upper"] = np.asarray(float(np.min(planner.root.value_upper)))
                store[p + "/rng_after"] = rng_state(planner.np_random)
                store[p + "/env_steps_total"] = np.asarray(len(planner.observations))
                n_steps += 1
                _, _, term, trunc, _ = env.step(plan[0])
                if term or trunc:
                    break
            store["{}/e{}/states".format(name, e)] = np.asarray(states, np.int64)
            store["{}/e{}/n_steps".format(name, e)] = np.asarray(n_steps)
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, len(store), "arrays", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
