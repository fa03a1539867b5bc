#!/usr/bin/env python3
"""Time the UNMODIFIED Python reference Sparse Sampling on the cases of tools/micro_sparse_sampling.py
-> profiles/sparse_sampling_reference_cpu.json.

The reference does not travel to the GPU machine, so this script -- run in the BUILD CONTAINER, the only place the
reference exists -- times ``SparseSamplingAgent.plan`` (tree_search/sparse_sampling.py:21-24) on the same tables and
configs, one core, through the adapters of make_golden_sparse_sampling.py; tools/micro_sparse_sampling.py states its kernel
times as a ratio to these.  Only ``plan()`` is timed: building the env and the agent is not the path.  Two columns: the
env's tables as nested lists, as an env built from the reference's JSON configs holds them (the deep copy per sample walks
them: ``s_per_plan``), and as numpy arrays (the deep copy is a memory copy: ``s_per_plan_arrays``).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/time_reference_sparse_sampling.py
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
from make_golden import agent_factory, np  # noqa: E402

REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, os.path.join(REPO, "tools"))
import micro_sparse_sampling  # noqa: E402

OUT = os.path.join(REPO, "profiles", "sparse_sampling_reference_cpu.json")
PLANS = 3


def main():
    rows = []
    for name, tab, cfg in micro_sparse_sampling.cases():
        S = np.asarray(tab["reward"]).shape[0]
        spent, spent_arrays, samples = [], [], 0
        for i in range(2 * PLANS):
            s0 = int(i % PLANS * 7919 % S)
            arrays = i >= PLANS
            env = gs.make_env(tab, s0) if arrays else gb.make_env(tab, s0)
            agent = agent_factory(gb.StaleApiEnv(env), dict(cfg, __class__=gs.SS))
            agent.seed(i % PLANS)
            agent.planner.np_random = gb.StaleGenerator(agent.planner.np_random.bit_generator)
            t = time.perf_counter()
            agent.plan(s0)
            (spent_arrays if arrays else spent).append(time.perf_counter() - t)
            if arrays:
                continue
            samples += sum(n.count for n, _ in agent.planner.root.breadth_first_search(agent.planner.root)
                           if not isinstance(n, gs.ref_ss.ChanceNode))
        row = dict(case=name, plans=PLANS, s_per_plan=float("{:.4g}".format(sorted(spent)[PLANS // 2])),
                   s_per_plan_arrays=float("{:.4g}".format(sorted(spent_arrays)[PLANS // 2])),
                   samples_per_plan=samples // PLANS, samples_per_s=float("{:.4g}".format(samples / sum(spent))), **cfg)
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(what="unmodified Python reference SparseSamplingAgent.plan, one core, median of %d plans; s_per_plan: the env holds "
                            "its tables as nested lists, s_per_plan_arrays: as numpy arrays" % PLANS,
                       host=platform.processor() or platform.machine(), python=platform.python_version(),
                       numpy=np.__version__, rows=rows), f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
