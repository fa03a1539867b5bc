#!/usr/bin/env python3
"""Time the UNMODIFIED Python reference Sparse Sampling on the shape and config of tests/golden/per_episode_sparse_sampling.npz
-> the "reference_cpu" entry of profiles/per_episode_sparse_sampling.json (the file's other entries are kept).

As time_reference_sparse_sampling.py: run in the BUILD CONTAINER, the only place the reference exists; only
``SparseSamplingAgent.plan`` (tree_search/sparse_sampling.py:21-24) is timed, one core, on highway-shaped (3, 4, 10) tables
with ``horizon 3, C 2, gamma 0.8``, through the adapters of make_golden_sparse_sampling.py.  Two columns: the env's tables as
nested lists (``s_per_plan``: the deep copy per sample walks them) and as numpy arrays (``s_per_plan_arrays``).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/time_reference_per_episode_sparse_sampling.py
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
import make_golden_sparse_sampling as gs  # noqa: E402
from make_golden import agent_factory, generators, np  # noqa: E402

REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
OUT = os.path.join(REPO, "profiles", "per_episode_sparse_sampling.json")
CONFIG = dict(horizon=3, C=2, gamma=0.8)
PLANS = 5


def main():
    spent, spent_arrays = [], []
    for i in range(2 * PLANS):
        k = i % PLANS
        tab = generators.highway_shaped(3, 4, 10, collision_rate=0.03 + 0.01 * k, seed=7000 + k)
        s0 = ((k % 3) * 4 + (k % 4)) * 10
        arrays = i >= PLANS
        env = gs.make_env(tab, s0) if arrays else gb.make_env(tab, s0)
        agent = agent_factory(gb.StaleApiEnv(env), dict(CONFIG, __class__=gs.SS))
        agent.seed(k)
        agent.planner.np_random = gb.StaleGenerator(agent.planner.np_random.bit_generator)
        t = time.perf_counter()
        agent.plan(s0)
        (spent_arrays if arrays else spent).append(time.perf_counter() - t)
    entry = dict(what="unmodified Python reference SparseSamplingAgent.plan, one core, median of %d plans on highway-shaped (3, 4, 10) "
                      "tables; s_per_plan: the env holds its tables as nested lists, s_per_plan_arrays: as numpy arrays" % PLANS,
                 host=platform.processor() or platform.machine(), python=platform.python_version(), numpy=np.__version__,
                 s_per_plan=float("{:.4g}".format(sorted(spent)[PLANS // 2])),
                 s_per_plan_arrays=float("{:.4g}".format(sorted(spent_arrays)[PLANS // 2])), **CONFIG)
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
