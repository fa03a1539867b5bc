#!/usr/bin/env python3
"""Time the UNMODIFIED Python reference GBOP on the cases of tools/micro_gbop.py -> profiles/gbop_reference_cpu.json.

The reference does not travel to the GPU machine, so this script -- run in the BUILD CONTAINER, the only place the reference
exists -- times ``StochasticGraphBasedPlannerAgent.plan`` (tree_search/graph_based_stochastic.py:332-337) with the parameters of
SailingEnv/agents/gbop.json and of the "GBOP" entry of scripts/planners_evaluation.py on finite-MDP envs of this package, one
core, through the adapters of make_golden_gbop.py.  The graph is kept from plan to plan: a planner's FIRST plan and its FOLLOWING
plans are timed separately, as tools/micro_gbop.py times the device.  Only ``plan()`` is timed.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/time_reference_gbop.py
"""
import json
import os
import platform
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_gbop as gg  # noqa: E402
from make_golden import agent_factory, np  # noqa: E402

REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, os.path.join(REPO, "tools"))
import micro_gbop  # noqa: E402

OUT = os.path.join(REPO, "profiles", "gbop_reference_cpu.json")
PLANNERS = 3
FOLLOWING = 3


def main():
    gg.install_adapter()
    rows = []
    for name, tab, agent_cfg in micro_gbop.cases():
        S = np.asarray(tab["reward"]).shape[0]
        first, following, steps = [], [], 0
        for i in range(PLANNERS):
            s0 = int(i * 7919 % S)
            env = gg.make_env(tab, s0)
            agent = agent_factory(gg.StaleApiEnv(env), dict(agent_cfg, __class__=gg.GBOP))
            agent.seed(i)
            agent.planner.np_random = gg.StaleGenerator(agent.planner.np_random.bit_generator)
            for rep in range(1 + FOLLOWING):
                s = (s0 + rep) % S
                env.mdp.state = s
                t = time.perf_counter()
                agent.plan(s)
                (first if rep == 0 else following).append(time.perf_counter() - t)
            steps += len(agent.planner.observations)
        med = lambda x: float("{:.4g}".format(sorted(x)[len(x) // 2]))  # noqa: E731
        row = dict(case=name, K=int(agent.planner.config["max_next_states_count"]), episodes=int(agent.planner.config["episodes"]),
                   horizon=int(agent.planner.config["horizon"]), planners=PLANNERS, following=FOLLOWING,
                   first_plan_s=med(first), first_plan_s_min=float("{:.4g}".format(min(first))),
                   following_plan_s=med(following), following_plan_s_min=float("{:.4g}".format(min(following))),
                   env_steps_per_s=float("{:.4g}".format(steps / (sum(first) + sum(following)))))
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(what="unmodified Python reference StochasticGraphBasedPlannerAgent.plan, one core, medians over %d planners "
                            "(first plan) and %d following plans each" % (PLANNERS, FOLLOWING),
                       host=platform.processor() or platform.machine(), python=platform.python_version(),
                       numpy=np.__version__, rows=rows), f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
