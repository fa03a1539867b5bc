#!/usr/bin/env python3
"""Time the UNMODIFIED Python reference MDP-GapE on the shape and the baseline config of tests/golden/per_episode_gape.npz
-> the "reference_cpu" entry of profiles/per_episode_gape.json (the file's other entries are kept).

As time_reference_per_episode_sparse_sampling.py: run in the BUILD CONTAINER, the only place the reference exists; only
``MDPGapEAgent.plan`` (tree_search/mdp_gape.py:94-110) is timed, one core, one episode's plan, on the fixture's highway-shaped
(3, 4, 10) tables (rewards clipped as there) with the reference's HighwayEnv/agents/MDPGapEAgent/baseline.json, through the
adapters of make_golden_olop.py.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/time_reference_per_episode_gape.py
"""
import json
import os
import platform
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_per_episode_gape import GAPE, StaleApiEnv, StaleGenerator, clipped, load_agent_json, table  # noqa: E402
from make_golden import agent_factory, np  # noqa: E402

from rl_agents_amd.envs import FiniteMDPEnv  # noqa: E402

REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
OUT = os.path.join(REPO, "profiles", "per_episode_gape.json")
PLANS = 7


def main():
    config = load_agent_json("HighwayEnv/agents/MDPGapEAgent/baseline.json")
    spent, episodes, horizon = [], None, None
    for e in range(PLANS):
        cfg = dict(clipped(table(e, 0)))
        cfg.pop("original_shape", None)
        cfg["state"] = ((e % 3) * 4 + (e % 4)) * 10
        env = FiniteMDPEnv(cfg)
        env.reset()
        agent = agent_factory(StaleApiEnv(env), dict(config, __class__=GAPE))
        agent.seed(100 + e)
        agent.planner.np_random = StaleGenerator(agent.planner.np_random.bit_generator)
        t = time.perf_counter()
        agent.plan(cfg["state"])
        spent.append(time.perf_counter() - t)
        episodes, horizon = int(agent.planner.config["episodes"]), int(agent.planner.config["horizon"])
    entry = dict(what="unmodified Python reference MDPGapEAgent.plan, one core, one episode's plan, median of %d plans on "
                      "highway-shaped (3, 4, 10) tables with HighwayEnv/agents/MDPGapEAgent/baseline.json" % PLANS,
                 host=platform.processor() or platform.machine(), python=platform.python_version(), numpy=np.__version__,
                 s_per_plan=float("{:.4g}".format(sorted(spent)[PLANS // 2])), episodes=episodes, horizon=horizon,
                 gamma=float(agent.planner.config["gamma"]), accuracy=float(agent.planner.config["accuracy"]))
    doc = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            doc = json.load(f)
    doc["reference_cpu"] = entry
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(entry))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
