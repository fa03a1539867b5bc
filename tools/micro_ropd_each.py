"""Robust OPD on one set of M models per root (mp_ropd_plan_models over mp_model_load_joint_batch) timed with HIP events
(ctx.last_kernel_ms) against mp_ropd_plan on one shared set, on this library and on the parent commit's.

    python tools/micro_ropd_each.py --parent-lib <the parent commit's libmi355plan.so> [--json profiles/ropd_each_micro.json]
    python tools/micro_ropd_each.py --loop [--json ...]

Shape: the highway shape, 120 states x 5 actions, M = 2 (the table and generators.rewire of it at 0.15); budgets 100 and 300,
gamma 0.8; 1, 256 and 4096 roots.  Three variants:
    a  the parent commit's library, mp_ropd_plan with every root on ONE shared set (mp_model_load_joint)
    b  this library, the same call
    c  this library, mp_ropd_plan_models with ONE SET PER ROOT (512 distinct sets, repeated)
Each variant runs in a process of its own (a library is loaded once per process) and is run TWICE, interleaved (a, b, c, a, b,
c); a run times every (roots, budget) as the median of 5 launches after a warm-up.  The spread between the two medians of one
variant is what a difference between variants has to exceed: b must equal a within a's spread (the kernels are the same); c has no
target, it is recorded with its ratio to a.  a and b are compared on their results on the way (checksums).
--loop: one PerEpisodeEvaluation.run() of the DiscreteRobustPlannerAgent at 256 ChangingHighwayEnv episodes, 10 steps, with where
its wall time went.
"""
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MI355PLAN_NO_TORCH", "1")
from rl_agents_amd.envs import generators  # noqa: E402

GAMMA, M = 0.8, 2
BUDGETS = [100, 300]
ROOTS = [1, 256, 4096]
DISTINCT = 512
NEW_SYMBOLS = ("mp_model_load_joint_batch", "mp_model_update_joint_tables", "mp_model_set_available_joint_batch", "mp_ropd_plan_models")


def model_set(k):
    base = generators.highway_shaped(3, 4, 10, collision_rate=0.03 + 0.01 * (k % 5), seed=7000 + k)
    other = generators.rewire(base, 0.15, seed=9000 + k)
    return (np.stack([base["transition"], other["transition"]]), np.stack([base["reward"], other["reward"]]),
            np.stack([base["terminal"], other["terminal"]]).astype(np.uint8))


def timed(ctx, call, base_rng):
    times, out = [], None
    for rep in range(6):
        out = call(base_rng.copy())
        ms, _ = ctx.last_kernel_ms()
        if rep > 0:
            times.append(ms)
    assert (out["status"] == 0).all()
    return statistics.median(times), min(times), max(times), ctx.last_kernel_variant(), out


def worker(variant):
    """One run of one variant: a JSON row per (roots, budget) on stdout."""
    from rl_agents_amd import native
    if variant == "a":
        for name in NEW_SYMBOLS:                 # (the parent commit's library does not export them)
            native.SIGNATURES.pop(name, None)
    ctx = native.Context(0)
    for n in ROOTS:
        local = (np.arange(n) * 37 % 120).astype(np.int32)
        base = native.seed_sequence_states((), 0, n)
        if variant == "c":
            sets = [model_set(k) for k in range(min(n, DISTINCT))]
            pick = np.arange(n) % len(sets)
            model = ctx.load_joint_batch(np.stack([s[0] for s in sets])[pick], np.stack([s[1] for s in sets])[pick],
                                         np.stack([s[2] for s in sets])[pick])
            mi = np.arange(n, dtype=np.int32)
        else:
            model, mi = ctx.load_joint(*model_set(0)), None
        for budget in BUDGETS:
            med, lo, hi, form, out = timed(ctx, lambda rng: ctx.ropd_plan(model, local, budget, GAMMA, 0.0, rng, max_plan_len=1,
                                                                          **({} if mi is None else dict(model_index=mi))), base)
            print(json.dumps(dict(variant=variant, roots=n, budget=budget, kernel_ms_median=round(med, 5), kernel_ms_min=round(lo, 5),
                                  kernel_ms_max=round(hi, 5), form=form, plans_checksum=int(np.asarray(out["plans"], np.int64).sum()),
                                  env_steps=int(out["env_steps"].sum()),
                                  lower_checksum=int(np.asarray(out["root_lower"]).view(np.uint64).sum(dtype=np.uint64) & np.uint64((1 << 62) - 1)))),
                  flush=True)
        model.close()
    ctx.close()


def run_variant(variant, parent_lib):
    env = dict(os.environ)
    if variant == "a":
        env["MI355PLAN_LIB"] = parent_lib
    else:
        env.pop("MI355PLAN_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", variant], env=env, stdout=subprocess.PIPE, check=True,
                         timeout=300).stdout.decode()
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def measure(parent_lib, out_path):
    runs = {v: [] for v in "abc"}
    for repeat in range(2):
        for v in "abc":
            runs[v].append({(r["roots"], r["budget"]): r for r in run_variant(v, parent_lib)})
    rows = []
    for n in ROOTS:
        for budget in BUDGETS:
            key = (n, budget)
            med = {v: [runs[v][k][key]["kernel_ms_median"] for k in range(2)] for v in "abc"}
            a, b, c = (statistics.mean(med[v]) for v in "abc")
            spread_a = abs(med["a"][0] - med["a"][1])
            ra, rb = runs["a"][0][key], runs["b"][0][key]
            same = all(ra[k] == rb[k] for k in ("plans_checksum", "env_steps", "lower_checksum", "form"))
            row = dict(measure="ropd_each", S_each=120, A=5, M=M, gamma=GAMMA, roots=n, budget=budget,
                       a_parent_shared_ms_medians=med["a"], b_this_shared_ms_medians=med["b"], c_each_ms_medians=med["c"],
                       spread_a_ms=round(spread_a, 5), spread_b_ms=round(abs(med["b"][0] - med["b"][1]), 5),
                       spread_c_ms=round(abs(med["c"][0] - med["c"][1]), 5), b_minus_a_ms=round(b - a, 5),
                       b_equals_a_within_spread_of_a=bool(abs(b - a) <= spread_a), b_over_a=round(b / a, 4), c_over_a=round(c / a, 4),
                       a_b_same_results=same, form_shared=ra["form"], form_each=runs["c"][0][key]["form"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    save(rows, out_path)


def save(rows, out_path):
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


def loop(out_path):
    from rl_agents_amd.agents.robust.robust import DiscreteRobustPlannerAgent
    from rl_agents_amd.envs import ChangingHighwayEnv
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    n = 256
    cfg = dict(budget=150, gamma=GAMMA, models=[[], [{"method": "with_collision_rate", "args": 0.15}]])
    envs = [ChangingHighwayEnv(3, 4, 10, table_seed=500 + 20 * i, state=((i % 3) * 4 + (i % 4)) * 10,
                               collision_rate=0.03 + 0.02 * (i % 4)) for i in range(n)]
    ev = PerEpisodeEvaluation(envs, DiscreteRobustPlannerAgent(envs[0], dict(cfg)), sim_seed=7, max_steps=10)
    out = ev.run()
    row = dict(measure="per_episode_loop", planner="ropd", M=M, budget=cfg["budget"], episodes=n, max_steps=10,
               env_steps=int(out["lengths"].sum()), wall_seconds=round(out["wall_seconds"], 4),
               seconds={k: round(v, 4) for k, v in out["seconds"].items()}, uploads=int(out["uploads"]),
               planner_env_steps=int(out["planner_env_steps"]), placement=ev.ctx.last_kernel_variant())
    ev.close()
    print(json.dumps(row), flush=True)
    rows = []
    if out_path and os.path.exists(out_path):
        with open(out_path) as f:
            rows = [r for r in json.load(f) if r.get("measure") != "per_episode_loop"]
    save(rows + [row], out_path)


def main():
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if "--variant" in sys.argv:
        return worker(sys.argv[sys.argv.index("--variant") + 1])
    if "--loop" in sys.argv:
        return loop(out_path)
    if "--parent-lib" not in sys.argv:
        sys.exit("--parent-lib <path of the parent commit's libmi355plan.so> is required (variant a)")
    measure(os.path.abspath(sys.argv[sys.argv.index("--parent-lib") + 1]), out_path)


if __name__ == "__main__":
    main()
