"""mp_gbopd_plan timed with HIP events (ctx.last_kernel_ms) on gridworld() and random_deterministic(1000, 4).

    python tools/micro_gbopd.py [--json profiles/gbopd_micro.json] [--planners 1,64,4096,65536] [--reps 5]

Per model, config (the default config at budget 400; budget 1000 / gamma 0.95) and batch size: a repetition makes a fresh
batch of planners, times its FIRST plan and three FOLLOWING plans on the kept graphs (every planner's root moves along
its own planned action in between); one warm-up repetition, then the median over ``--reps``.  Reported: ms per plan call,
plans / s, queue pops / s and expansions / s (both counted by the kernel's own outputs: ``updates`` and the growth of
the expanded nodes of up to 64 exported planners, scaled), and the kernel form ("gbopd_wave_lds": both bounds in LDS).
Where profiles/gbopd_reference_cpu.json (tests/golden/gen/time_reference_gbopd.py: the unmodified Python reference, one
core) has the (model, config), its ms per plan ride along with the ratios reference / device for one plan and per planner
of the batch.  Registers and spills: python tools/kernel_resources.py rl_agents_amd/csrc/gbopd.hip gbopd.
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

PLANNERS = [1, 64, 4096, 65536]
MODELS = [("gridworld", lambda: generators.gridworld()),
          ("random_deterministic_1000x4", lambda: generators.random_deterministic(1000, 4, seed=0))]
CONFIGS = [("default_b400", dict(budget=400, gamma=0.8, accuracy=1e-2, sampling_timeout=100)),
           ("b1000_g095", dict(budget=1000, gamma=0.95, accuracy=1e-2, sampling_timeout=100))]
REFERENCE = os.path.join(ROOT, "profiles", "gbopd_reference_cpu.json")
FOLLOWING = 3


def arg_list(flag, default):
    if flag in sys.argv:
        return [int(x) for x in sys.argv[sys.argv.index(flag) + 1].split(",")]
    return default


def one_repetition(native, ctx, model, T, n, cfg):
    """A fresh batch: (ms, pops, expansions of the sampled planners) of the first and of each following plan."""
    S = T.shape[0]
    handle = native.GraphBasedPlanners(ctx, model, n)
    roots = (np.arange(n) * 7919 % S).astype(np.int32)
    rng = native.seed_sequence_states((), 0, n)
    sample = range(min(n, 64))
    expanded, plans = [0] * len(sample), []
    for _ in range(1 + FOLLOWING):
        out = handle.plan(roots, cfg["budget"], cfg["gamma"], 1 / (1 - cfg["gamma"]), cfg["accuracy"], cfg["sampling_timeout"], rng)
        ms, _ = ctx.last_kernel_ms()
        assert (out["status"] == 0).all()
        now = [int(handle.export(i)["expanded"].sum()) for i in sample]
        plans.append((ms, int(out["updates"].sum()), (sum(now) - sum(expanded)) * n / len(sample)))
        expanded = now
        act = np.maximum(out["plans"][:, 0], 0)
        roots = T[roots, act].astype(np.int32)
    variant, qcap = ctx.last_kernel_variant(), handle.info()["queue_cap"]
    handle.close()
    return plans, variant, qcap


def main():
    from rl_agents_amd import native
    reference = {}
    if os.path.exists(REFERENCE):
        with open(REFERENCE) as f:
            reference = {(r["model"], r["config"]): r for r in json.load(f)["rows"]}
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    reps = arg_list("--reps", [5])[0]
    ctx = native.Context(0)
    rows = []
    for mname, make in MODELS:
        tab = make()
        T = np.asarray(tab["transition"])
        model = ctx.load_table(tab["transition"], tab["reward"], tab["terminal"])
        for cname, cfg in CONFIGS:
            for n in arg_list("--planners", PLANNERS):
                runs = [one_repetition(native, ctx, model, T, n, cfg) for _ in range(1 + reps)][1:]
                variant, qcap = runs[0][1], runs[0][2]
                first = statistics.median(r[0][0][0] for r in runs)
                follow = statistics.median(statistics.mean(p[0] for p in r[0][1:]) for r in runs)
                pops_first, exp_first = runs[0][0][0][1], runs[0][0][0][2]
                pops_follow = sum(p[1] for p in runs[0][0][1:]) / FOLLOWING
                exp_follow = sum(p[2] for p in runs[0][0][1:]) / FOLLOWING
                g = lambda x: float("{:.4g}".format(x))  # noqa: E731
                row = dict(model=mname, config=cname, S=int(T.shape[0]), A=int(T.shape[1]), planners=n, kernel=variant, queue_cap=qcap,
                           reps=reps, first_plan_ms=round(first, 4), following_plan_ms=round(follow, 4),
                           first_plan_ms_min_max=[round(min(r[0][0][0] for r in runs), 4), round(max(r[0][0][0] for r in runs), 4)],
                           first_plans_per_s=g(n / (first * 1e-3)), following_plans_per_s=g(n / (follow * 1e-3)),
                           first_pops_per_s=g(pops_first / (first * 1e-3)), following_pops_per_s=g(pops_follow / (follow * 1e-3)),
                           first_expansions_per_s=g(exp_first / (first * 1e-3)), following_expansions_per_s=g(exp_follow / (follow * 1e-3)),
                           pops_per_first_plan=g(pops_first / n), pops_per_following_plan=g(pops_follow / n))
                ref = reference.get((mname, cname))
                if ref is not None:
                    ref_first = ref["first_plan"]["ms"]
                    ref_follow = statistics.mean(p["ms"] for p in ref["following_plans"])
                    row.update(reference_first_plan_ms=ref_first, reference_following_plan_ms=round(ref_follow, 3),
                               reference_over_device_first_per_planner=g(ref_first / (first / n)),
                               reference_over_device_following_per_planner=g(ref_follow / (follow / n)))
                rows.append(row)
                print(json.dumps(row), flush=True)
                if out_path:
                    with open(out_path, "w") as f:
                        json.dump(rows, f, indent=1)
                        f.write("\n")
        model.close()
    ctx.close()


if __name__ == "__main__":
    main()
