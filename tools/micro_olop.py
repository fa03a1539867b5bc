"""mp_olop_plan timed with HIP events (ctx.last_kernel_ms) on the reference's OLOP configs and a highway-shaped table.

    python tools/micro_olop.py [--json OUT]

Per shape and root count: kernel ms (best of 3 after a warm-up), env steps per second (episodes * horizon per root), and
where the trees lived ("olop_global": one per root, "olop_global_slots": one per workgroup).  Registers and spills:
python tools/kernel_resources.py rl_agents_amd/csrc/olop.hip olop.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MI355PLAN_NO_TORCH", "1")
from rl_agents_amd import native  # noqa: E402
from rl_agents_amd.agents.tree_search.olop import OLOP  # noqa: E402
from rl_agents_amd.envs import generators  # noqa: E402

SHAPES = [
    # name, table, budget, gamma, bound threshold (KL, global time), continuation
    ("gridworld_kl_b500_g0.8", generators.gridworld(), 500, 0.8, "4*np.log(time)", -1),
    ("finitemdp_kl_b100_g0.9", generators.random_deterministic(30, 3, seed=41), 100, 0.9, "4*np.log(time)", 0),
    ("highway_S10000_A5_kl_b500_g0.7", generators.highway_shaped(10, 10, 100, seed=0), 500, 0.7, "2*np.log(time)", -1),
]
ROOTS = [1, 256, 4096, 65536]


def main():
    ctx = native.Context(0)
    rows = []
    for name, tab, budget, gamma, thr_expr, cont in SHAPES:
        reward = np.clip(tab["reward"], 0.0, 1.0)
        model = ctx.load_table(tab["transition"], reward, tab["terminal"])
        S, A = reward.shape
        episodes, horizon = OLOP.allocation(max(A, budget), gamma)
        thr = np.full(episodes, float(eval(thr_expr, {"np": np}, {"time": episodes})))
        vinit = OLOP.value_upper_init(gamma, horizon)
        for n in ROOTS:
            roots = (np.arange(n) * 7919 % S).astype(np.int32)
            base = native.seed_sequence_states((), 0, n)
            best, variant = None, None
            for rep in range(4):
                rng = base.copy()
                out = ctx.olop_plan(model, roots, episodes, horizon, gamma, True, cont, thr, vinit, rng)
                ms, _ = ctx.last_kernel_ms()
                variant = ctx.last_kernel_variant()
                assert (out["status"] == 0).all()
                if rep > 0:
                    best = ms if best is None else min(best, ms)
            steps = n * episodes * horizon
            row = dict(shape=name, S=S, A=A, episodes=episodes, horizon=horizon, roots=n, kernel_ms=round(best, 4),
                       env_steps_per_s=float("{:.4g}".format(steps / (best * 1e-3))), placement=variant)
            rows.append(row)
            print(json.dumps(row), flush=True)
        model.close()
    ctx.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
