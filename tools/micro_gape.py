"""mp_gape_plan timed with HIP events (ctx.last_kernel_ms) on the default MDP-GapE config and on the highway baseline's.

    python tools/micro_gape.py [--json profiles/gape_micro.json]

Cases (``cases()``, which tests/golden/gen/time_reference_gape.py times the reference on, too): the default config (budget 500,
gamma 0.8, accuracy 1, confidence 0.9, the default threshold) on a random table of S = 100, |A| = 5, and the config of
HighwayEnv/agents/MDPGapEAgent/baseline.json (budget 100, gamma 0.8, accuracy 0.1, threshold "1*np.log(time)") on a
highway-shaped table of 3 speeds, 4 lanes and 10 time slices.  Per case and root count: kernel ms (the median of SAMPLES calls
after a warm-up call, with the smallest and largest sample), the episodes run and model steps per second, and the kernel form.
Nothing is asserted but the status.  Registers and spills: python tools/kernel_resources.py rl_agents_amd/csrc/gape.hip gape.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MI355PLAN_NO_TORCH", "1")
from rl_agents_amd.envs import generators  # noqa: E402

ROOTS = [1, 256, 4096]
SAMPLES = 5


def cases():
    """name, finite-MDP config, agent config."""
    return [("default_S100_A5", generators.random_deterministic(100, 5, seed=53), dict(budget=500, gamma=0.8)),
            ("highway_3x4x10", generators.highway_shaped(3, 4, 10, seed=3),
             dict(gamma=0.8, budget=100, accuracy=0.1, confidence=1, max_next_states_count=1, continuation_type="uniform",
                  step_strategy="reset", upper_bound=dict(type="kullback-leibler", time="global", threshold="1*np.log(time)")))]


def main():
    from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapEAgent
    from rl_agents_amd.envs import FiniteMDPEnv
    rows = []
    for name, table, agent_cfg in cases():
        S = np.asarray(table["reward"]).shape[0]
        env = FiniteMDPEnv(dict(mode="deterministic", transition=np.asarray(table["transition"]).tolist(),
                                reward=np.asarray(table["reward"]).tolist(),
                                terminal=np.asarray(table["terminal"]).astype(int).tolist(), state=0))
        env.reset()
        planner = MDPGapEAgent(env, dict(agent_cfg)).planner
        ctx = planner.models.ctx
        for n in ROOTS:
            roots = (np.arange(n) * 7919 % S).astype(np.int32)
            base = planner.batch_rng_states(n)
            samples, variant = [], None
            for rep in range(SAMPLES + 1):
                out = planner.plan_batch(env, roots, rng_states=base.copy())
                ms, _ = ctx.last_kernel_ms()
                variant = ctx.last_kernel_variant()
                assert (out["status"] == 0).all()
                if rep > 0:
                    samples.append(ms)
            med = float(np.median(samples))
            row = dict(case=name, S=S, A=int(np.asarray(table["reward"]).shape[1]), episodes=int(planner.config["episodes"]),
                       horizon=int(planner.config["horizon"]), roots=n, samples=SAMPLES, kernel_ms=round(med, 4),
                       kernel_ms_min=round(min(samples), 4), kernel_ms_max=round(max(samples), 4),
                       episodes_run_mean=float("{:.4g}".format(out["episodes_run"].mean())),
                       env_steps_per_s=float("{:.4g}".format(int(out["env_steps"].sum()) / (med * 1e-3))), placement=variant)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
