"""The rule uct_kernel's virgin groups rest on (csrc/uct_virgin.hpp), pinned on the CPU oracle's trees.  No GPU.

In the tree of a FRESH plan without phantom slots a node expands on its first visit only, so
    count == 1 and first_child >= 0   =>   every child is {value 0.0, count 0, first_child -1}
    count >= 2 and first_child >= 0   =>   at least one child was visited (count >= 1)
and a node with children has count >= 1.  The first line is what the kernel, the export, the re-rooting and mp_uct_path_count
use; it holds in re-rooted trees too, where the second does not (a node can expand late: its depth and step count changed) --
which is why only fresh-tree plans leave groups unstored.

A seeded set of 600 fresh plans: |A| 2..8, horizons 1..30, 1..80 episodes, tables of 4..40 states with terminal states, both done
rules, step limits with a non-zero start step.  Then plans that continue re-rooted trees: the first line again, and a count of
the late expansions that break the second."""
import numpy as np

ZERO = (0.0, 0, -1)


def check_parents(tree, k, both_directions):
    """-> (parents checked, parents that break the second line)"""
    cnt, val, fc = tree["count"], tree["value"], tree["first_child"]
    parents, late = 0, 0
    for node in np.flatnonzero(fc >= 0):
        kids = slice(int(fc[node]), int(fc[node]) + k)
        parents += 1
        assert cnt[node] >= 1, "a node with children was visited"
        if cnt[node] == 1:
            assert (cnt[kids] == 0).all() and (val[kids] == 0.0).all() and (fc[kids] == -1).all(), \
                "node {} has count 1 and a child that is not {}".format(node, ZERO)
        elif (cnt[kids] == 0).all():
            late += 1
            assert not both_directions, "node {} has count {} and no visited child".format(node, cnt[node])
    return parents, late


def draw_case(g):
    from rl_agents_amd.envs import generators
    k, horizon, episodes = int(g.integers(2, 9)), int(g.integers(1, 31)), int(g.integers(1, 81))
    n_states = int(g.integers(4, 41))
    cfg = generators.random_deterministic(n_states, k, int(g.integers(1 << 30)), terminal_rate=float(g.choice([0.0, 0.1, 0.4])))
    rule = "next" if g.integers(2) else "source"
    max_steps = int(g.choice([0, 0, 3, 7, 15]))
    steps0 = int(g.integers(0, max_steps)) if max_steps else 0
    return dict(k=k, horizon=horizon, episodes=episodes, n_states=n_states, cfg=cfg, rule=rule, max_steps=max_steps, steps0=steps0)


def plan(c, s0, steps0, rng, init_tree=None):
    from oracle import oracle
    p = np.ones(c["k"]) / c["k"]
    return oracle.uct_plan(c["cfg"]["transition"], c["cfg"]["reward"], c["cfg"]["terminal"], s0, c["episodes"], c["horizon"], 0.9, 5.0, p, p,
                           rng, steps0=steps0, max_steps=c["max_steps"], done_rule=c["rule"], max_plan_len=4, init_tree=init_tree)


def test_rule_on_fresh_plans():
    from rl_agents_amd import native
    g = np.random.Generator(np.random.PCG64(2024))
    rngs = native.seed_sequence_states((), 31000, 600)
    parents, count1 = 0, 0
    for i in range(600):
        c = draw_case(g)
        tree = plan(c, int(g.integers(c["n_states"])), c["steps0"], rngs[i])["tree"]
        n, _ = check_parents(tree, c["k"], both_directions=True)
        parents += n
        count1 += int(((tree["count"] == 1) & (tree["first_child"] >= 0)).sum())
    assert parents >= 4000 and count1 >= 2000, (parents, count1)     # (the set is not made of trivial trees)


def test_first_line_holds_in_re_rooted_trees_the_second_does_not():
    from oracle import oracle
    from rl_agents_amd import native
    g = np.random.Generator(np.random.PCG64(2025))
    rngs = native.seed_sequence_states((), 32000, 200)
    late = 0
    for i in range(200):
        c = draw_case(g)
        s = int(g.integers(c["n_states"]))
        out = plan(c, s, c["steps0"], rngs[i])
        for step in range(3):
            a = int(g.integers(c["k"]))
            kept = oracle.uct_reroot(out["tree"], a, c["k"])
            s = int(c["cfg"]["transition"][s, a])
            out = plan(c, s, c["steps0"], out["rng_after"], init_tree=kept)
            late += check_parents(out["tree"], c["k"], both_directions=False)[1]
    assert late > 0, "no late expansion in the set: the second line was not put to the test"
