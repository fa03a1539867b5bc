"""The cases of the sweep of MDP-GapE with transition bounds on one MDP per root (tests/test_gpu_each_gape_stoch.py;
tests/test_each_gape_stoch_host.py checks on the CPU what they contain and how many of their plans the margin rule of
tests/gape_cases.py leaves out) -- no GPU needed.

Case i < N_CASES takes shape, mask, listing order, done rule, K and planner config from ``gape_stoch_cases.random_case(3 * i)`` --
the deterministic-table cases of that sweep; masks fall on 3 i % 4 == 1, permuted listing orders on 3 i % 8 == 1 -- and plans on
TABLES tables of its own: table k is ``generators.random_deterministic(S, A, seed=SEED_TABLE + 10 * i + k, terminal_rate=0.2 if
k % 2 else 0.0)`` with rewards clipped to [1e-3, 1 - 1e-3]; where the base case is masked, table k gets a mask of its own,
``random_available(S, A, seed=SEED_MASK + 10 * i + k, rate=0.4)`` -- a form that reads the flags of another table lists other
actions.  One root per table: states and generator records from ``default_rng(SEED_ROOTS + i)``."""
import numpy as np

from rl_agents_amd.envs import generators
from tests import gape_stoch_cases as gsc

N_CASES = 19
TABLES = 5
SEED_TABLE, SEED_MASK, SEED_ROOTS = 9500, 9700, 9900
PLANNER_KEYS = ("horizon", "episodes", "gamma", "accuracy", "continuation", "threshold", "max_next_states_count",
                "transition_threshold")


def each_case(i):
    """-> dict(base, tables [TABLES] of golden-layout cases (one per table, restate_plan reads them), model_index, local, rng)."""
    base = gsc.random_case(3 * i)
    assert str(base["mdp/mode"]) == "deterministic"
    n_states, n_actions = base["mdp/reward"].shape
    masked = (3 * i) % 4 == 1
    planner = {k: base[k] for k in PLANNER_KEYS}
    rng = np.random.default_rng(SEED_ROOTS + i)
    local = rng.integers(0, n_states, size=TABLES).astype(np.int32)
    records = gsc.records(rng, TABLES)
    tables = []
    for k in range(TABLES):
        cfg = gsc.table("deterministic", n_states, n_actions, 0, SEED_TABLE + 10 * i + k, 0.2 if k % 2 else 0.0)
        available = generators.random_available(n_states, n_actions, seed=SEED_MASK + 10 * i + k, rate=0.4) if masked else None
        tables.append(gsc.pack(cfg, available, base["order"], base["done_on_next"], local[k:k + 1], records[k:k + 1], **planner))
    return dict(base=base, tables=tables, masked=masked, model_index=np.arange(TABLES, dtype=np.int32), local=local, rng=records)


def restate_each(case):
    """The restatement on every root's OWN table alone -> [(result, generator record after, margin)]."""
    out = []
    for k in range(TABLES):
        res, after, seen = gsc.restate_plan(case["tables"][k], int(case["local"][k]), case["rng"][k])
        out.append((res, after, gsc.margin(seen)))
    return out


def device_tables(tables):
    """(transition [N,S,A], reward, terminal [N,S], available [N*S,A], action_column [A]) as the entry point takes them: the
    device's columns are the environment's actions in listing order."""
    order = np.asarray(tables[0]["order"])
    t = np.stack([c["mdp/transition"] for c in tables]).astype(np.int64)[:, :, order]
    r = np.stack([c["mdp/reward"] for c in tables]).astype(np.float64)[:, :, order]
    term = np.stack([np.asarray(c["mdp/terminal"]) for c in tables]).astype(np.uint8)
    available = np.stack([c["available"] for c in tables])[:, :, order].reshape(-1, len(order))
    column = np.empty(len(order), np.int32)
    column[order] = np.arange(len(order))
    return t, r, term, available, column
