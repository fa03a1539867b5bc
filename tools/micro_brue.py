"""mp_brue_plan timed with HIP events (ctx.last_kernel_ms) on a deterministic, a sparse and a dense model.

    python tools/micro_brue.py [--json profiles/brue_micro.json] [--roots 1,256,4096,65536] [--budgets 300,1000]

Per model, budget and root count: kernel ms (median of 5 after a warm-up), env steps per second (the steps the plans
took), nodes per tree (mean over up to 64 exported trees), and where the trees lived ("brue_global": one per root,
"brue_global_slots": one per workgroup).  Where profiles/brue_reference_cpu.json (tests/golden/gen/time_reference_brue.py:
the unmodified Python reference on the same tables, one core) has the shape, its seconds per plan ride along with the
ratio reference time per plan / device time per plan of the batch.  Registers and spills:
python tools/kernel_resources.py rl_agents_amd/csrc/brue.hip brue.
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MI355PLAN_NO_TORCH", "1")
from rl_agents_amd.envs import generators  # noqa: E402

GAMMA = 0.8
BUDGETS = [300, 1000]
ROOTS = [1, 256, 4096, 65536]
REFERENCE = os.path.join(ROOT, "profiles", "brue_reference_cpu.json")


def shapes():
    """name -> finite-MDP config (shared with the reference timer)."""
    return [("highway_det_S10000_A5", generators.highway_shaped(10, 10, 100, seed=0)),
            ("sparse_S1000_A5_B3", generators.random_sparse(1000, 5, 3, seed=1, terminal_rate=0.02)),
            ("dense_S64_A4", generators.random_stochastic(64, 4, seed=2, terminal_rate=0.02))]


def load(ctx, tab):
    if tab["mode"] == "deterministic":
        return ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
    if tab["mode"] == "sparse":
        return ctx.load_sparse(tab["transition"], tab["next"], tab["reward"], tab["terminal"])
    return ctx.load_dense(tab["transition"], tab["reward"], tab["terminal"])


def arg_list(flag, default):
    if flag in sys.argv:
        return [int(x) for x in sys.argv[sys.argv.index(flag) + 1].split(",")]
    return default


def main():
    from rl_agents_amd import native
    from rl_agents_amd.agents.tree_search.brue import BRUE
    reference = {}
    if os.path.exists(REFERENCE):
        with open(REFERENCE) as f:
            reference = {(r["shape"], r["budget"]): r for r in json.load(f)["rows"]}
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    ctx = native.Context(0)
    rows = []
    for name, tab in shapes():
        model = load(ctx, tab)
        S, A = np.asarray(tab["reward"]).shape
        for budget in arg_list("--budgets", BUDGETS):
            _, horizon = BRUE.allocation(max(A, budget), GAMMA)
            gpow = BRUE.gamma_powers(GAMMA, horizon)
            for n in arg_list("--roots", ROOTS):
                roots = (np.arange(n) * 7919 % S).astype(np.int32)
                base = native.seed_sequence_states((), 0, n)
                times, variant, steps = [], None, 0
                for rep in range(6):
                    out = ctx.brue_plan(model, roots, budget, horizon, GAMMA, gpow, base.copy())
                    ms, _ = ctx.last_kernel_ms()
                    variant = ctx.last_kernel_variant()
                    assert (out["status"] == 0).all() and (out["plans"] >= 0).all()
                    steps = int(out["env_steps"].sum())
                    if rep > 0:
                        times.append(ms)
                cap = 1 + 2 * (budget + horizon)
                exportable = range(min(n, 64)) if variant == "brue_global" else [0]
                nodes = float(np.mean([len(ctx.brue_tree(i, cap)["parent"]) for i in exportable]))
                med = statistics.median(times)
                row = dict(shape=name, mode=tab["mode"], S=S, A=A, budget=budget, horizon=horizon, gamma=GAMMA, roots=n,
                           kernel_ms_median=round(med, 4), kernel_ms_min=round(min(times), 4), kernel_ms_max=round(max(times), 4),
                           runs=len(times), env_steps_per_s=float("{:.4g}".format(steps / (med * 1e-3))),
                           nodes_per_tree=round(nodes, 1), placement=variant)
                ref = reference.get((name, budget))
                if ref is not None:
                    row["reference_python_s_per_plan"] = ref["s_per_plan"]
                    row["reference_over_device_per_plan"] = float("{:.4g}".format(ref["s_per_plan"] / (med * 1e-3 / n)))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if out_path:
                    with open(out_path, "w") as f:
                        json.dump(rows, f, indent=1)
        model.close()
    ctx.close()


if __name__ == "__main__":
    main()
