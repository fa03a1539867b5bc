#!/usr/bin/env python3
"""Time the UNMODIFIED Python reference MDP-GapE on the cases of tools/micro_gape_stoch.py ->
profiles/gape_stoch_reference_cpu.json.

The reference does not travel to the GPU machine, so this script -- run in the BUILD CONTAINER, the only place the reference
exists -- times ``MDPGapEAgent.plan`` (tree_search/mdp_gape.py:94-110) with ``max_next_states_count`` 2 and 8 on the same
models and config, one core, through the adapters of make_golden_gape_stoch.py; DESIGN.md states the single-root kernel times of
profiles/gape_stoch_micro.json as a ratio to these.  Only ``plan()`` is timed: building the env and the agent is not the path.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/time_reference_gape_stoch.py
"""
import json
import os
import platform
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_gape_stoch as gg  # noqa: E402
from make_golden import agent_factory, np  # noqa: E402

REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, os.path.join(REPO, "tools"))
import micro_gape_stoch  # noqa: E402

OUT = os.path.join(REPO, "profiles", "gape_stoch_reference_cpu.json")
PLANS = 5


def main():
    rows = []
    for name, tab, agent_cfg in micro_gape_stoch.cases():
        S = np.asarray(tab["reward"]).shape[0]
        spent, steps, episodes = [], 0, []
        for i in range(PLANS):
            s0 = int(i * 7919 % S)
            env = gg.make_env(tab, s0)
            agent = agent_factory(gg.StaleApiEnv(env), dict(agent_cfg, __class__=gg.GAPE))
            agent.seed(i)
            agent.planner.np_random = gg.StaleGenerator(agent.planner.np_random.bit_generator)
            t = time.perf_counter()
            agent.plan(s0)
            spent.append(time.perf_counter() - t)
            steps += len(agent.planner.observations)
            episodes.append(agent.planner.budget_used // agent.planner.config["horizon"])
        row = dict(case=name, K=int(agent.planner.config["max_next_states_count"]), episodes=int(agent.planner.config["episodes"]),
                   horizon=int(agent.planner.config["horizon"]), plans=PLANS, episodes_run=episodes,
                   s_per_plan=float("{:.4g}".format(sorted(spent)[PLANS // 2])), s_per_plan_min=float("{:.4g}".format(min(spent))),
                   env_steps_per_s=float("{:.4g}".format(steps / sum(spent))))
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(what="unmodified Python reference MDPGapEAgent.plan, one core, median of %d plans" % PLANS,
                       host=platform.processor() or platform.machine(), python=platform.python_version(),
                       numpy=np.__version__, rows=rows), f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
