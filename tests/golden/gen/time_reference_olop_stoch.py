#!/usr/bin/env python3
"""Time the UNMODIFIED Python reference OLOP on the two stochastic models of tools/micro_olop_stoch.py ->
profiles/olop_stoch_reference_cpu.json.

The reference does not travel to the GPU machine, so this script -- run in the BUILD CONTAINER, the only place the reference
exists -- times ``OLOP.plan`` (tree_search/olop.py:94-100) on the same models with the same default-config KL-OLOP (budget
500, gamma 0.8), one core, through the adapters of make_golden_brue.py.  Only ``plan()`` is timed: building the env and the
agent is not the path.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/time_reference_olop_stoch.py
"""
import json
import os
import platform
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_brue as gb  # noqa: E402
from make_golden import agent_factory, np  # noqa: E402

REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, os.path.join(REPO, "tools"))
import micro_olop_stoch  # noqa: E402

OUT = os.path.join(REPO, "profiles", "olop_stoch_reference_cpu.json")
OLOP = "<class 'rl_agents.agents.tree_search.olop.OLOPAgent'>"
PLANS = 5


def main():
    rows = []
    for name, tab in micro_olop_stoch.shapes():
        if tab["mode"] == "deterministic":
            continue
        spent, steps = [], 0
        for i in range(PLANS):
            s0 = int(i * 7919 % micro_olop_stoch.S)
            env = gb.make_env(tab, s0)
            agent = agent_factory(gb.StaleApiEnv(env), {"__class__": OLOP, "budget": micro_olop_stoch.BUDGET,
                                                        "gamma": micro_olop_stoch.GAMMA,
                                                        "upper_bound": {"type": "kullback-leibler"}})
            agent.seed(i)
            agent.planner.np_random = gb.StaleGenerator(agent.planner.np_random.bit_generator)
            t = time.perf_counter()
            agent.plan(s0)
            spent.append(time.perf_counter() - t)
            steps += len(agent.planner.observations)
        pc = agent.planner.config
        row = dict(shape=name, budget=micro_olop_stoch.BUDGET, gamma=micro_olop_stoch.GAMMA, episodes=pc["episodes"],
                   horizon=pc["horizon"], plans=PLANS, s_per_plan=float("{:.4g}".format(sorted(spent)[PLANS // 2])),
                   env_steps_per_s=float("{:.4g}".format(steps / sum(spent))))
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(what="unmodified Python reference OLOP.plan (KL-OLOP, budget 500, gamma 0.8), one core, median of %d plans"
                            % PLANS, host=platform.processor() or platform.machine(), python=platform.python_version(),
                       numpy=np.__version__, rows=rows), f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
