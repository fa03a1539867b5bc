"""mp_ss_plan timed with HIP events (ctx.last_kernel_ms) on a deterministic, a sparse and a dense model.

    python tools/micro_sparse_sampling.py [--json profiles/sparse_sampling_micro.json] [--roots 1,256,4096,65536]

Per case and root count: kernel ms (median of 5 after a warm-up), samples (model steps) per second, nodes per tree (mean
over up to 64 exported trees) and the kernel form ("ss_wave_lds" / "ss_wave_global").  The cases are the reference's shipped
config (gamma 0.7, horizon 3, C 3) on the three model kinds and a sparse A = 5, horizon 3, C 5 shape.  Where
profiles/sparse_sampling_reference_cpu.json (tests/golden/gen/time_reference_sparse_sampling.py: the unmodified Python
reference on the same tables, one core) has the case, its seconds per plan ride along with the ratio reference time per
plan / device time per plan of the batch, for both of its env representations (tables as nested lists / as arrays); the
single-root row is the one to compare a plan with a plan.  The last level is taken in one pass over the lanes; the A/B
against taking it action by action, from the build that still had both, is profiles/sparse_sampling_last_level_ab.json.
Registers and spills:
python tools/kernel_resources.py rl_agents_amd/csrc/sparse_sampling.hip ss_kernel.
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

ROOTS = [1, 256, 4096, 65536]
REFERENCE = os.path.join(ROOT, "profiles", "sparse_sampling_reference_cpu.json")
SHIPPED = dict(gamma=0.7, horizon=3, C=3)


def cases():
    """name, finite-MDP config, planner config (shared with the reference timer)."""
    return [("det_S30_A3_shipped", generators.random_deterministic(30, 3, seed=81), SHIPPED),
            ("sparse_S60_A3_B2_shipped", generators.random_sparse(60, 3, 2, seed=85), SHIPPED),
            ("dense_S20_A3_shipped", generators.random_stochastic(20, 3, seed=83), SHIPPED),
            ("sparse_S50_A5_B3_h3_C5", generators.random_sparse(50, 5, 3, seed=86, terminal_rate=0.15), dict(gamma=0.7, horizon=3, C=5))]


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
    reference = {}
    if os.path.exists(REFERENCE):
        with open(REFERENCE) as f:
            reference = {r["case"]: r for r in json.load(f)["rows"]}
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    ctx = native.Context(0)
    rows = []
    for name, tab, cfg in cases():
        model = load(ctx, tab)
        S, A = np.asarray(tab["reward"]).shape
        for n in arg_list("--roots", ROOTS):
            roots = (np.arange(n) * 7919 % S).astype(np.int32)
            base = native.seed_sequence_states((), 0, n)
            times, variant, samples = [], None, 0
            for rep in range(6):
                out = ctx.ss_plan(model, roots, cfg["horizon"], cfg["C"], cfg["gamma"], base.copy())
                ms, _ = ctx.last_kernel_ms()
                variant = ctx.last_kernel_variant()
                assert (out["status"] == 0).all() and (out["plans"] >= 0).all()
                samples = int(out["samples"].sum())
                if rep > 0:
                    times.append(ms)
            try:
                nodes = float(np.mean([len(ctx.ss_tree(i)["parent"]) for i in range(min(n, 64))]))
                kept = "every root"
            except native.NativeError:
                nodes, kept = float(len(ctx.ss_tree(0)["parent"])), "root 0"
            med = statistics.median(times)
            row = dict(case=name, mode=tab["mode"], S=S, A=A, horizon=cfg["horizon"], C=cfg["C"], gamma=cfg["gamma"], roots=n,
                       kernel_ms_median=round(med, 4), kernel_ms_min=round(min(times), 4), kernel_ms_max=round(max(times), 4),
                       runs=len(times), samples_per_plan=samples // n, samples_per_s=float("{:.4g}".format(samples / (med * 1e-3))),
                       nodes_per_tree=round(nodes, 1), trees_kept=kept, form=variant)
            ref = reference.get(name)
            if ref is not None:
                # (two reference columns: its env holding the tables as nested lists / as arrays, whose deep copy is cheaper)
                for key, tag in (("s_per_plan", ""), ("s_per_plan_arrays", "_arrays")):
                    row["reference_python_s_per_plan" + tag] = ref[key]
                    row["reference%s_over_device_per_plan" % tag] = float("{:.4g}".format(ref[key] / (med * 1e-3 / n)))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(rows, f, indent=1)
        model.close()
    ctx.close()


if __name__ == "__main__":
    main()
