"""MDP-GapE with transition bounds on one MDP per root (mp_gape_plan_stochastic_models) timed with HIP events
(ctx.last_kernel_ms): the root's table in LDS ("gape_stoch_each_lds") against the batch model's records in global memory
("gape_stoch_each_global").

    python tools/micro_gape_stoch_each.py [--json profiles/gape_stoch_each_ab.json] [--roots 1,256,4096,65536]

Shape: the highway shape, 120 states x 5 actions (9.6 KB of records a table), ONE TABLE PER ROOT (512 distinct tables, repeated),
rewards clipped to [1e-3, 1 - 1e-3]; the "k2" config of tests/golden/per_episode_gape_stoch.npz: horizon 3, 20 episodes, gamma
0.8, accuracy 0, max_next_states_count 2, both thresholds by their default strings ("1*np.log(time)", "0.1*np.log(time)"),
uniform continuation.  Per batch size every form is timed TWICE, interleaved in one process (global, lds, global, lds), each time
the median of 5 runs after a warm-up: the spread between the two medians of one form is what a difference between the forms has
to exceed.  The results of the two forms are compared bit for bit on the way.  With --json, rows of another ``measure`` already in
the file are kept.
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MI355PLAN_NO_TORCH", "1")
from micro_each import arg_list, highway_batch  # noqa: E402
from micro_gape_each import same, timed  # noqa: E402

GAMMA, HORIZON, EPISODES, ACCURACY, K = 0.8, 3, 20, 0.0, 2
ROOTS = [1, 256, 4096, 65536]


def save_rows(rows, out_path, measure="forms"):
    if not out_path:
        return
    kept = []
    if os.path.exists(out_path):
        with open(out_path) as f:
            kept = [r for r in json.load(f) if r.get("measure") != measure]
    with open(out_path, "w") as f:
        json.dump(kept + rows, f, indent=1)


def forms(ctx, rows, out_path):
    from rl_agents_amd import native
    cus = ctx.device_info()["n_cu"]
    names = ["lds", "global"]
    thr = np.full(EPISODES + 2, float(1 * np.log(EPISODES)))            # "1*np.log(time)", time = the number of episodes
    tthr = np.full(EPISODES + 2, float(0.1 * np.log(EPISODES)))         # "0.1*np.log(time)"
    vin = np.array([(1 - GAMMA ** (HORIZON - d)) / (1 - GAMMA) for d in range(HORIZON + 1)])
    for n in arg_list("--roots", ROOTS):
        t, r, term = highway_batch(n)
        model = ctx.load_table_batch(t, np.clip(r, 1e-3, 1 - 1e-3), term)
        mi = np.arange(n, dtype=np.int32)
        local = (np.arange(n) * 37 % 120).astype(np.int32)
        base = native.seed_sequence_states((), 0, n)
        med, outs = {name: [] for name in names}, {}
        for repeat in range(2):
            for form in reversed(names):
                os.environ["MP_EACH_MODEL"] = form
                m, lo, hi, variant, out = timed(ctx, lambda rng: ctx.gape_plan_stochastic_models(
                    model, mi, local, EPISODES, HORIZON, K, GAMMA, ACCURACY, True, 5, None, thr, tthr, vin, rng), base)
                assert variant.startswith("gape_stoch_each_" + form), variant
                med[form].append(m)
                outs[form] = (out, variant, lo, hi)
        del os.environ["MP_EACH_MODEL"]
        info = native.gape_stoch_each_form_info(120, 5, HORIZON, n, cus)
        row = dict(measure="forms", planner="gape_stoch", S_each=120, A=5, horizon=HORIZON, episodes=EPISODES, gamma=GAMMA,
                   accuracy=ACCURACY, max_next_states_count=K, roots=n,
                   spread_ms=round(max(abs(v[0] - v[1]) for v in med.values()), 4),
                   default_form="lds" if info["lds"] else "global", variants=[outs[f][1] for f in names],
                   plans_checksum=int(np.asarray(outs[names[0]][0]["plans"], np.int64).sum()),
                   episodes_run=int(outs[names[0]][0]["episodes_run"].sum()), env_steps=int(outs[names[0]][0]["env_steps"].sum()))
        for form in names:
            row[form + "_ms_medians"] = [round(x, 4) for x in med[form]]
        assert same(outs["global"][0], outs["lds"][0]), "the two forms differ"
        g, l = statistics.mean(med["global"]), statistics.mean(med["lds"])
        os.environ["MP_EACH_MODEL"] = "lds"
        lds_info = native.gape_stoch_each_form_info(120, 5, HORIZON, n, cus)
        del os.environ["MP_EACH_MODEL"]
        row.update(lds_over_global=round(l / g, 4), lds_wins_beyond_spread=bool(g - l > row["spread_ms"]), bit_identical=True,
                   lds_bytes_per_workgroup=lds_info["lds_bytes"], lds_waves_per_cu=min(32, (160 * 1024) // lds_info["lds_bytes"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        save_rows(rows, out_path)
        model.close()


def main():
    from rl_agents_amd import native
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    rows = []
    ctx = native.Context(0)
    forms(ctx, rows, out_path)
    ctx.close()


if __name__ == "__main__":
    main()
