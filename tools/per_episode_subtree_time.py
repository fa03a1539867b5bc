#!/usr/bin/env python3
"""Plan time per lock-step of PerEpisodeEvaluation with MCTS that keeps its subtrees, beside step_strategy "reset", from ONE run.

    python tools/per_episode_subtree_time.py [--episodes 4096] [--steps 6] [--out profiles/per_episode_subtree.json]

A kept-tree plan does not run on the LDS-resident forms (they start from fresh trees): state-independent policies on an
unrestricted environment continue on `uct_global`; restricted action sets and prior agents plan, from the first step on, with
the kernel that stores priors and child sets at expansion (mp_uct_plan_stochastic_policy).  Two environments, MCTSAgent budget
1000 (33 x 30) as bench.py's per_episode_eval:

    restricted    ChangingHighwayEnv: a (3, 4, 10) grid re-drawn after every step, restricted action sets listed IDLE first
    unrestricted  ScheduledTableEnv over highway-shaped tables (a pool of 64, each episode walking it from its own offset)

`plan_ms` is the loop's own split (seconds["plan"]: launches + results + the synchronisation) per lock-step; the first lock-step
(model and policy built, workspaces allocated, fresh trees in both strategies) is reported apart from the mean of the others.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def make_envs(kind, n, steps):
    from rl_agents_amd.envs import ChangingHighwayEnv, ScheduledTableEnv, generators
    if kind == "restricted":
        return [ChangingHighwayEnv(3, 4, 10, table_seed=20 * i, state=((i % 3) * 4 + (i % 4)) * 10, collision_rate=0.03 + 0.02 * (i % 4))
                for i in range(n)]
    pool = [{k: v for k, v in generators.highway_shaped(3, 4, 10, collision_rate=0.03 + 0.02 * (j % 4), seed=9000 + j).items()
             if k != "original_shape"} for j in range(64)]
    return [ScheduledTableEnv([pool[(7 * i + t) % 64] for t in range(steps)], state=((i % 3) * 4 + (i % 4)) * 10) for i in range(n)]


def timed_run(kind, strategy, n, steps):
    from rl_agents_amd.agents.tree_search.mcts import MCTSAgent
    from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
    envs = make_envs(kind, n, steps)
    agent = MCTSAgent(envs[0], dict(budget=1000, gamma=0.8, horizon=30, episodes=33, step_strategy=strategy))
    ev = PerEpisodeEvaluation(envs, agent, sim_seed=1, max_steps=steps)
    plan_s, forms, live = [], [], []
    real = ev._plan

    def plan(idx, states, step_counts):
        ev.ctx.synchronize()
        t0 = time.perf_counter()
        out = real(idx, states, step_counts)
        ev.ctx.synchronize()
        plan_s.append(time.perf_counter() - t0)
        forms.append(ev.ctx.last_kernel_variant())
        live.append(len(idx))
        return out
    ev._plan = plan
    t0 = time.perf_counter()
    out = ev.run()
    wall = time.perf_counter() - t0
    ev.close()
    lock_steps = len(plan_s)
    return dict(strategy=strategy, lock_steps=lock_steps, live_per_lock_step=live, kernel_forms=forms,
                plan_ms_per_lock_step=[1e3 * s for s in plan_s], plan_ms_first=1e3 * plan_s[0],
                plan_ms_mean_after_first=1e3 * float(np.mean(plan_s[1:])) if lock_steps > 1 else None,
                wall_ms_per_lock_step=1e3 * wall / max(lock_steps, 1),
                split_ms_per_lock_step={k: 1e3 * v / max(lock_steps, 1) for k, v in out["seconds"].items()},
                episode_steps=int(out["lengths"].sum()), planner_env_steps=int(out["planner_env_steps"]),
                mean_return=float(out["returns"].mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(episodes=args.episodes, steps=args.steps, agent="MCTSAgent budget 1000 (33 x 30), gamma 0.8", kinds={})
    for kind in ("restricted", "unrestricted"):
        res["kinds"][kind] = {s: timed_run(kind, s, args.episodes, args.steps) for s in ("reset", "subtree")}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
