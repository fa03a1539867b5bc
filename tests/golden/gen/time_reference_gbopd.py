#!/usr/bin/env python3
"""Wall time of the UNMODIFIED reference GraphBasedPlannerAgent (through the two adapters of make_golden_gbopd.py) on the
models and configs of tools/micro_gbopd.py, one CPU core: the baseline the device numbers are quoted against.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/time_reference_gbopd.py      (build container only)
-> profiles/gbopd_reference_cpu.json

Per (model, config): the first plan of a fresh agent and three following plans on the kept graph (the environment steps
the planned action in between), each with its wall time, its queue pops (the growth of sum(get_updates())) and its
expansions (the growth of the number of expanded nodes).
"""
import json
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_gbopd as mg  # noqa: E402
from make_golden import agent_factory, generators  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "..", "..", "profiles", "gbopd_reference_cpu.json"))
MODELS = {"gridworld": lambda: generators.gridworld(), "random_deterministic_1000x4": lambda: generators.random_deterministic(1000, 4, seed=0)}
CONFIGS = {"default_b400": dict(budget=400), "b1000_g095": dict(budget=1000, gamma=0.95)}


def main():
    mg.install_adapter()
    rows = []
    for mname, make in MODELS.items():
        for cname, cfg in CONFIGS.items():
            env = mg.make_env(make(), 0)
            agent = agent_factory(mg.StaleApiEnv(env), dict(cfg, __class__=mg.GBOPD))
            agent.seed(0)
            planner = agent.planner
            plans = []
            for k in range(4):
                pops0 = sum(planner.get_updates().values())
                exp0 = sum(1 for n in planner.nodes.values() if n.children)
                t0 = time.perf_counter()
                a = agent.act(env.mdp.state)
                dt = time.perf_counter() - t0
                plans.append(dict(ms=round(dt * 1e3, 3), pops=sum(planner.get_updates().values()) - pops0,
                                  expansions=sum(1 for n in planner.nodes.values() if n.children) - exp0,
                                  nodes=len(planner.nodes)))
                env.step(a)
            rows.append(dict(model=mname, config=cname, first_plan=plans[0], following_plans=plans[1:]))
            print(mname, cname, plans, flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(what="reference GraphBasedPlannerAgent, one CPU core, parents in insertion order", rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
