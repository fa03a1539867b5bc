"""mp_gape_plan_stochastic timed with HIP events (ctx.last_kernel_ms) on the reference's FiniteMDPEnv MDP-GapE config.

    python tools/micro_gape_stoch.py [--json profiles/gape_stoch_micro.json]

Cases (``cases()``, which tests/golden/gen/time_reference_gape_stoch.py times the reference on, too): the config of
FiniteMDPEnv/agents/mdp-gape.json (gamma 0.7, budget 100, accuracy 0, confidence 1, threshold "1*np.log(time)",
max_next_states_count 2) on the tables of the golden cases of tests/golden/gen/make_golden_gape_stoch.py -- a sparse model of
12 states with 2 successors, a dense model of 8 states with max_next_states_count 8, and a deterministic table of 20 states.
Per case and root count: kernel ms (the median of SAMPLES calls after a warm-up call, with the smallest and largest sample), the
episodes run and model steps per second, and the kernel form.  Nothing is asserted but the status.
profiles/gape_stoch_solves_ab.json holds this script's figures for the library and for a variant of the backup loop that is not
kept in the source (one solve after the other in lanes 0..31), taken alternating in one session through MI355PLAN_LIB.
Registers and spills: python tools/kernel_resources.py rl_agents_amd/csrc/gape_stoch.hip gape.
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
FINITE = dict(gamma=0.7, budget=100, accuracy=0.0, confidence=1.0, max_next_states_count=2, continuation_type="uniform",
              upper_bound=dict(type="kullback-leibler", time="global", threshold="1*np.log(time)"))


def cases():
    """name, finite-MDP config, agent config."""
    return [("finite_sparse_b2", dict(generators.random_sparse(12, 3, 2, seed=101), mode="sparse"), dict(FINITE)),
            ("finite_dense8_k8", dict(generators.random_stochastic(8, 3, seed=102), mode="stochastic"),
             dict(FINITE, max_next_states_count=8)),
            ("finite_det_k2", dict(generators.random_deterministic(20, 3, seed=103), mode="deterministic"), dict(FINITE))]


def env_config(table, state=0):
    cfg = dict(mode=table["mode"], transition=np.asarray(table["transition"]).tolist(), reward=np.asarray(table["reward"]).tolist(),
               terminal=np.asarray(table["terminal"]).astype(int).tolist(), state=int(state))
    if table["mode"] == "sparse":
        cfg["next"] = np.asarray(table["next"]).tolist()
    return cfg


def main():
    from rl_agents_amd.agents.tree_search.mdp_gape import StochasticMDPGapEAgent
    from rl_agents_amd.envs import FiniteMDPEnv
    rows = []
    for name, table, agent_cfg in cases():
        S = np.asarray(table["reward"]).shape[0]
        env = FiniteMDPEnv(env_config(table))
        env.reset()
        planner = StochasticMDPGapEAgent(env, dict(agent_cfg)).planner
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
            row = dict(case=name, S=S, A=int(np.asarray(table["reward"]).shape[1]), K=int(planner.config["max_next_states_count"]),
                       episodes=int(planner.config["episodes"]), horizon=int(planner.config["horizon"]), roots=n, samples=SAMPLES,
                       kernel_ms=round(med, 4), kernel_ms_min=round(min(samples), 4), kernel_ms_max=round(max(samples), 4),
                       episodes_run_mean=float("{:.4g}".format(out["episodes_run"].mean())),
                       env_steps_per_s=float("{:.4g}".format(int(out["env_steps"].sum()) / (med * 1e-3))), placement=variant)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
