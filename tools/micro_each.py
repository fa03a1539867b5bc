"""OLOP and BRUE on one MDP per root (mp_olop_plan_models / mp_brue_plan_models) timed with HIP events (ctx.last_kernel_ms):
the root's table in LDS ("..._each_lds") against the batch model's records in global memory ("..._each_global").

    python tools/micro_each.py [--json profiles/each_model_ab.json] [--roots 1,256,4096,65536]
    MI355PLAN_LIB=<the parent commit's library> python tools/micro_each.py --baseline [--json ...]
    python tools/micro_each.py --loop [--json ...]

Shape: the highway shape, 120 states x 5 actions (9.6 KB of records a table), ONE TABLE PER ROOT (512 distinct tables, repeated);
budgets: the default-config budgets of profiles/olop_micro.json (KL-OLOP, 500) and profiles/brue_micro.json (300), gamma 0.8.
Per planner and batch size every form is timed TWICE, interleaved (global, lds, global, lds), each time the median of 5 runs
after a warm-up: the spread between the two medians of one form is what a difference between the forms has to exceed.  The
results of the two forms are compared bit for bit on the way.  A second shape whose table does not fit LDS (4000 states x 3
actions, 192 KB) shows the chooser falling back to the global form.

--baseline (run on the parent commit's library, which has neither entry point): OLOP = mp_olop_plan on the same batch model
addressed by global states (bit-identical results); BRUE = mp_brue_plan with all roots on ONE table of the shape (mp_brue_plan
refuses batch models: its footprint is one table, not one per root).
--loop: one PerEpisodeEvaluation.run() at 256 ChangingHighwayEnv episodes per planner, with where its wall time went.
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
BUDGET = dict(olop=500, brue=300)
ROOTS = [1, 256, 4096, 65536]
DISTINCT = 512
NEW_SYMBOLS = ("mp_olop_plan_models", "mp_brue_plan_models", "mp_each_form_info", "mp_each_form_names")


def arg_list(flag, default):
    if flag in sys.argv:
        return [int(x) for x in sys.argv[sys.argv.index(flag) + 1].split(",")]
    return default


def highway_batch(n):
    tabs = [generators.highway_shaped(3, 4, 10, collision_rate=0.03 + 0.01 * (k % 5), seed=7000 + k) for k in range(min(n, DISTINCT))]
    pick = np.arange(n) % len(tabs)
    return (np.stack([t["transition"] for t in tabs])[pick], np.stack([t["reward"] for t in tabs])[pick],
            np.stack([t["terminal"] for t in tabs]).astype(np.uint8)[pick])


def planner_args(planner):
    from rl_agents_amd import native
    from rl_agents_amd.agents.tree_search.brue import BRUE
    from rl_agents_amd.agents.tree_search.olop import OLOP
    episodes, horizon = native.olop_allocation(BUDGET[planner], GAMMA)
    if planner == "olop":
        thr = np.full(episodes, float(4 * np.log(episodes)))
        return dict(episodes=episodes, horizon=horizon, thr=thr, vinit=OLOP.value_upper_init(GAMMA, horizon))
    return dict(horizon=horizon, gpow=BRUE.gamma_powers(GAMMA, horizon))


def plan(ctx, planner, model, a, states, rng, model_index=None):
    if planner == "olop":
        return ctx.olop_plan(model, states, a["episodes"], a["horizon"], GAMMA, True, -1, a["thr"], a["vinit"], rng, max_plan_len=1,
                             **({} if model_index is None else dict(model_index=model_index)))
    return ctx.brue_plan(model, states, BUDGET[planner], a["horizon"], GAMMA, a["gpow"], rng,
                         **({} if model_index is None else dict(model_index=model_index)))


def timed(ctx, call, base_rng):
    """Median of 5 kernel times after a warm-up -> (median, min, max, the form that ran, the last result)."""
    times, out = [], None
    for rep in range(6):
        out = call(base_rng.copy())
        ms, _ = ctx.last_kernel_ms()
        if rep > 0:
            times.append(ms)
    assert (out["status"] == 0).all()
    return statistics.median(times), min(times), max(times), ctx.last_kernel_variant(), out


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in ("plans", "root_value", "env_steps"))


def save(rows, out_path):
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


def forms(ctx, rows, out_path):
    from rl_agents_amd import native
    cus = ctx.device_info()["n_cu"]
    for n in arg_list("--roots", ROOTS):
        t, r, term = highway_batch(n)
        model = ctx.load_table_batch(t, r, term)
        mi = np.arange(n, dtype=np.int32)
        local = (np.arange(n) * 37 % 120).astype(np.int32)
        base = native.seed_sequence_states((), 0, n)
        for planner in ("olop", "brue"):
            a = planner_args(planner)
            med, outs = {"global": [], "lds": []}, {}
            for repeat in range(2):
                for form in ("global", "lds"):
                    os.environ["MP_EACH_MODEL"] = form
                    m, lo, hi, variant, out = timed(ctx, lambda rng: plan(ctx, planner, model, a, local, rng, mi), base)
                    assert variant.startswith("{}_each_{}".format(planner, form)), variant
                    med[form].append(m)
                    outs[form] = (out, variant, lo, hi)
            del os.environ["MP_EACH_MODEL"]
            assert same(outs["global"][0], outs["lds"][0]), "the two forms differ"
            info = native.each_form_info(planner, 120, 5, a["horizon"], n, cus)
            g, l = statistics.mean(med["global"]), statistics.mean(med["lds"])
            spread = max(abs(med["global"][0] - med["global"][1]), abs(med["lds"][0] - med["lds"][1]))
            row = dict(measure="forms", planner=planner, S_each=120, A=5, budget=BUDGET[planner], horizon=a["horizon"], gamma=GAMMA, roots=n,
                       global_ms_medians=[round(x, 4) for x in med["global"]], lds_ms_medians=[round(x, 4) for x in med["lds"]],
                       spread_ms=round(spread, 4), lds_over_global=round(l / g, 4), lds_wins_beyond_spread=bool(g - l > spread),
                       placement_global=outs["global"][1], placement_lds=outs["lds"][1], lds_bytes_per_workgroup=info["lds_bytes"],
                       lds_waves_per_cu=min(32, (160 * 1024) // info["lds_bytes"]), default_form="lds" if info["lds"] else "global",
                       bit_identical=True, plans_checksum=int(np.asarray(outs["lds"][0]["plans"], np.int64).sum()),
                       env_steps=int(outs["lds"][0]["env_steps"].sum()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            save(rows, out_path)
        model.close()
    # a table that does not fit LDS: the chooser falls back, also when the knob asks for LDS
    tabs = [generators.random_deterministic(4000, 3, seed=k, terminal_rate=0.02) for k in range(4)]
    model = ctx.load_table_batch(np.stack([x["transition"] for x in tabs]), np.stack([x["reward"] for x in tabs]),
                                 np.stack([x["terminal"] for x in tabs]).astype(np.uint8))
    n = 256
    mi, local = (np.arange(n) % 4).astype(np.int32), (np.arange(n) * 37 % 4000).astype(np.int32)
    base = native.seed_sequence_states((), 0, n)
    for planner in ("olop", "brue"):
        a = planner_args(planner)
        for knob in (None, "lds"):
            if knob:
                os.environ["MP_EACH_MODEL"] = knob
            m, lo, hi, variant, _ = timed(ctx, lambda rng: plan(ctx, planner, model, a, local, rng, mi), base)
            os.environ.pop("MP_EACH_MODEL", None)
            assert variant.startswith(planner + "_each_global"), variant
            row = dict(measure="does_not_fit", planner=planner, S_each=4000, A=3, budget=BUDGET[planner], roots=n, knob=knob or "",
                       lds_bytes_per_workgroup=native.each_form_info(planner, 4000, 3, a["horizon"], n, cus)["lds_bytes"],
                       kernel_ms_median=round(m, 4), placement=variant)
            rows.append(row)
            print(json.dumps(row), flush=True)
    save(rows, out_path)
    model.close()


def baseline(ctx, rows, out_path):
    from rl_agents_amd import native
    for n in arg_list("--roots", ROOTS):
        base = native.seed_sequence_states((), 0, n)
        local = (np.arange(n) * 37 % 120).astype(np.int32)
        t, r, term = highway_batch(n)
        batch = ctx.load_table_batch(t, r, term)
        one = ctx.load_table(t[0], r[0], term[0])
        for planner, model, states, what in (("olop", batch, (np.arange(n) * 120 + local).astype(np.int32), "mp_olop_plan, batch model, global states"),
                                             ("brue", one, local, "mp_brue_plan, every root on ONE table")):
            a = planner_args(planner)
            meds = []
            for repeat in range(2):
                m, lo, hi, variant, out = timed(ctx, lambda rng: plan(ctx, planner, model, a, states, rng), base)
                meds.append(m)
            row = dict(measure="baseline", planner=planner, what=what, budget=BUDGET[planner], horizon=a["horizon"], roots=n,
                       kernel_ms_medians=[round(x, 4) for x in meds], placement=variant,
                       plans_checksum=int(np.asarray(out["plans"], np.int64).sum()), env_steps=int(out["env_steps"].sum()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            save(rows, out_path)
        batch.close()
        one.close()


def loop(rows, out_path):
    from rl_agents_amd.agents.tree_search.brue import BRUEAgent
    from rl_agents_amd.agents.tree_search.olop import OLOPAgent
    from rl_agents_amd.envs import ChangingHighwayEnv
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    n = 256
    cfgs = dict(olop=(OLOPAgent, {"budget": BUDGET["olop"], "gamma": GAMMA, "upper_bound": {"type": "kullback-leibler"},
                                  "continuation_type": "uniform"}),
                brue=(BRUEAgent, {"budget": BUDGET["brue"], "gamma": GAMMA}))
    for planner, (cls, cfg) in cfgs.items():
        envs = [ChangingHighwayEnv(3, 4, 10, table_seed=500 + 20 * i, state=((i % 3) * 4 + (i % 4)) * 10,
                                   collision_rate=0.03 + 0.02 * (i % 4)) for i in range(n)]
        ev = PerEpisodeEvaluation(envs, cls(envs[0], dict(cfg)), sim_seed=7, max_steps=10)
        out = ev.run()
        row = dict(measure="per_episode_loop", planner=planner, episodes=n, max_steps=10, env_steps=int(out["lengths"].sum()),
                   wall_seconds=round(out["wall_seconds"], 4), seconds={k: round(v, 4) for k, v in out["seconds"].items()},
                   uploads=int(out["uploads"]), planner_env_steps=int(out["planner_env_steps"]), placement=ev.ctx.last_kernel_variant())
        ev.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    save(rows, out_path)


def main():
    from rl_agents_amd import native
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    rows = []
    if "--loop" in sys.argv:
        return loop(rows, out_path)
    if "--baseline" in sys.argv:
        for name in NEW_SYMBOLS:                 # (the parent commit's library does not export them)
            native.SIGNATURES.pop(name, None)
    ctx = native.Context(0)
    (baseline if "--baseline" in sys.argv else forms)(ctx, rows, out_path)
    ctx.close()


if __name__ == "__main__":
    main()
