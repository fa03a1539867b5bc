"""mp_olop_plan_stochastic timed with HIP events (ctx.last_kernel_ms) on default-config KL-OLOP (budget 500, gamma 0.8).

    python tools/micro_olop_stoch.py [--json profiles/olop_stoch_micro.json]

Models: a sparse B = 3 model and a dense model of S = 100, |A| = 5 (rl_agents_amd/envs/generators.py), and -- the line to read
each number against, timed in the same run -- mp_olop_plan on a deterministic table of the same S and |A|.  Per model and root
count: kernel ms (the median of SAMPLES calls after a warm-up call, with the smallest and largest sample), env steps per second
(episodes * horizon per root) and the kernel form.  Nothing is asserted but the status.  Registers and spills:
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

S, A, BUDGET, GAMMA = 100, 5, 500, 0.8
ROOTS = [1, 256, 4096, 65536]
SAMPLES = 5


def shapes():
    """name, finite-MDP config: what tests/golden/gen/time_reference_olop_stoch.py times the reference on, too."""
    return [("sparse_S100_A5_B3", generators.random_sparse(S, A, 3, seed=51)),
            ("dense_S100_A5", generators.random_stochastic(S, A, seed=52)),
            ("table_S100_A5", generators.random_deterministic(S, A, seed=53))]


def load(ctx, cfg):
    if cfg["mode"] == "deterministic":
        return ctx.load_table(cfg["transition"], cfg["reward"], cfg["terminal"])
    if cfg["mode"] == "sparse":
        return ctx.load_sparse(cfg["transition"], cfg["next"], cfg["reward"], cfg["terminal"])
    return ctx.load_dense(cfg["transition"], cfg["reward"], cfg["terminal"])


def main():
    ctx = native.Context(0)
    episodes, horizon = OLOP.allocation(max(A, BUDGET), GAMMA)
    thr = np.full(episodes, 4 * np.log(episodes))
    vinit = OLOP.value_upper_init(GAMMA, horizon)
    rows = []
    for name, cfg in shapes():
        model = load(ctx, cfg)
        plan = ctx.olop_plan if cfg["mode"] == "deterministic" else ctx.olop_plan_stochastic
        for n in ROOTS:
            roots = (np.arange(n) * 7919 % S).astype(np.int32)
            base = native.seed_sequence_states((), 0, n)
            samples, variant = [], None
            for rep in range(SAMPLES + 1):
                rng = base.copy()
                out = plan(model, roots, episodes, horizon, GAMMA, True, 0, thr, vinit, rng)     # "zeros", the default
                ms, _ = ctx.last_kernel_ms()
                variant = ctx.last_kernel_variant()
                assert (out["status"] == 0).all()
                if rep > 0:
                    samples.append(ms)
            med = float(np.median(samples))
            row = dict(shape=name, S=S, A=A, episodes=episodes, horizon=horizon, roots=n, samples=SAMPLES, kernel_ms=round(med, 4),
                       kernel_ms_min=round(min(samples), 4), kernel_ms_max=round(max(samples), 4),
                       env_steps_per_s=float("{:.4g}".format(n * episodes * horizon / (med * 1e-3))), placement=variant)
            rows.append(row)
            print(json.dumps(row), flush=True)
        model.close()
    ctx.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
