"""mp_gbop_plan timed with HIP events (ctx.last_kernel_ms) on the reference's own GBOP configs.

    python tools/micro_gbop.py [--json profiles/gbop_micro.json]

Cases (``cases()``, which tests/golden/gen/time_reference_gbop.py times the reference on, too): the parameters of
SailingEnv/agents/gbop.json (budget 1000, gamma 0.9, max_next_states_count 3) and of the "GBOP" entry of
scripts/planners_evaluation.py (default budget 500, gamma 0.8, accuracy 5e-2, max_next_states_count 3), each on a sparse model
of 30 states, 4 actions and 3 successors a row, and the second on a deterministic table too.
The graph is KEPT from plan to plan, so a planner's first plan (an empty graph) and its following plans (a graph that holds
most states already) are timed separately: per case and planner count a fresh handle is made SAMPLES times for the first plan,
and FOLLOWING further plans are made on the last one; each figure is the median, with the smallest and largest sample.  The
kernel form (with the placement of the bounds) is recorded with every number.
The reference's partial value iteration does not end on every input, and among 4 096 planners some meet such
an input: the pop limit of a plan is lowered to MAX_POPS here (MP_GBOP_MAX_POPS; a million pops for the single planner, whose
figure is the one the README compares), the planners that hit it are counted per row
(``diverged``; they stay failed, so the following plans are fast for them) and every other status is asserted to be MP_OK.
Registers and spills: python tools/kernel_resources.py rl_agents_amd/csrc/gbop.hip gbop.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MI355PLAN_NO_TORCH", "1")
from rl_agents_amd.envs import generators  # noqa: E402

PLANNERS = [1, 4096]
SAMPLES = 5
FOLLOWING = 5
MAX_POPS = {1: 1000000, 4096: 20000}          # the pop limit of a plan by planner count (the library's own is 2^22)
ZERO = dict(type="kullback-leibler", threshold="0*np.log(time)", transition_threshold="0.1*np.log(time)")
SAILING = dict(budget=1000, gamma=0.9, upper_bound=dict(ZERO), max_next_states_count=3)
EVALUATION = dict(gamma=0.8, upper_bound=dict(ZERO), max_next_states_count=3, accuracy=5e-2)


def cases():
    """name, finite-MDP config, agent config."""
    sparse = dict(generators.random_sparse(30, 4, 3, seed=301), mode="sparse")
    det = dict(generators.random_deterministic(30, 4, seed=302), mode="deterministic")
    return [("sailing_config_sparse", sparse, dict(SAILING)), ("evaluation_config_sparse", sparse, dict(EVALUATION)),
            ("evaluation_config_table", det, dict(EVALUATION))]


def env_config(table, state=0):
    cfg = dict(mode=table["mode"], transition=np.asarray(table["transition"]).tolist(), reward=np.asarray(table["reward"]).tolist(),
               terminal=np.asarray(table["terminal"]).astype(int).tolist(), state=int(state))
    if table["mode"] == "sparse":
        cfg["next"] = np.asarray(table["next"]).tolist()
    return cfg


def main():
    from rl_agents_amd.agents.tree_search.graph_based_stochastic import StochasticGraphBasedPlannerAgent
    from rl_agents_amd import native
    from rl_agents_amd.envs import FiniteMDPEnv
    rows = []
    for name, table, agent_cfg in cases():
        S = np.asarray(table["reward"]).shape[0]
        env = FiniteMDPEnv(env_config(table))
        env.reset()
        planner = StochasticGraphBasedPlannerAgent(env, dict(agent_cfg)).planner
        ctx = planner.models.ctx
        for n in PLANNERS:
            os.environ["MP_GBOP_MAX_POPS"] = str(MAX_POPS[n])
            roots = (np.arange(n) * 7919 % S).astype(np.int32)
            base = planner.batch_rng_states(n)
            first, following, variant, steps, diverged = [], [], None, 0, 0
            planner.defer_errors = True                         # (statuses are read here)
            fine = lambda out: np.isin(out["status"], (native.MP_OK, native.MP_ERR_GBOPD_DIVERGED)).all()  # noqa: E731
            for rep in range(SAMPLES + 1):                      # (the first call is the warm-up)
                planner.forget()
                out = planner.plan_batch(env, roots, rng_states=base.copy())
                assert fine(out), out["status"]
                if rep > 0:
                    first.append(ctx.last_kernel_ms()[0])
            for rep in range(FOLLOWING):
                out = planner.plan_batch(env, (roots + rep + 1) % S, rng_states=base.copy())
                assert fine(out), out["status"]
                diverged = int((out["status"] != native.MP_OK).sum())
                following.append(ctx.last_kernel_ms()[0])
                variant, steps = ctx.last_kernel_variant(), int(out["env_steps"].sum())
            planner.forget()
            row = dict(case=name, S=S, A=int(np.asarray(table["reward"]).shape[1]), K=int(planner.config["max_next_states_count"]),
                       episodes=int(planner.config["episodes"]), horizon=int(planner.config["horizon"]), planners=n, samples=SAMPLES,
                       first_plan_ms=round(float(np.median(first)), 4), first_plan_ms_min=round(min(first), 4),
                       first_plan_ms_max=round(max(first), 4), following_plan_ms=round(float(np.median(following)), 4),
                       following_plan_ms_min=round(min(following), 4), following_plan_ms_max=round(max(following), 4),
                       env_steps_per_s=float("{:.4g}".format(steps / (float(np.median(following)) * 1e-3))), placement=variant,
                       diverged=diverged, max_pops=MAX_POPS[n], pops_per_planner=float("{:.4g}".format(out["pops"].mean())))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
