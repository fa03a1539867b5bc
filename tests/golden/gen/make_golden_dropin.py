#!/usr/bin/env python3
"""Golden records for the drop-in tests that used to import the reference at test time
(tests/test_dropin_reference_factory.py, tests/test_tree_tools.py::test_reference_tree_plot_draws_this_packages_tree).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_dropin.py <reference checkout>

-> tests/golden/reference_factory.json: what the UNMODIFIED reference's classes and factory return -- default_config() of
   every agent class the package mirrors, and the agent / planner config of an agent its agent_factory built from
   {"__class__": ..., "budget": 60, "gamma": 0.75}.  Before writing, the reference's own load_agent is run on a JSON
   file that names this package's class instead, and must build this package's agent.
-> tests/golden/reference_tree_plot.json: the segments the reference's TreePlot draws for two trees of
   tests/golden/tree_tools.npz rebuilt as this package's Node tree (x0, y0, x1, y1, line width; rounded to 9 digits).
Nothing of the reference is copied: its outputs only.
"""
import importlib
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
GOLDEN = os.path.abspath(os.path.join(HERE, ".."))

# (reference class, this package's class) -- the pairs tests/test_dropin_reference_factory.py checks
AGENTS = [
    ("rl_agents.agents.tree_search.mcts.MCTSAgent", "rl_agents_amd.agents.tree_search.mcts.MCTSAgent"),
    ("rl_agents.agents.tree_search.deterministic.DeterministicPlannerAgent",
     "rl_agents_amd.agents.tree_search.deterministic.DeterministicPlannerAgent"),
    ("rl_agents.agents.tree_search.state_aware.StateAwarePlannerAgent",
     "rl_agents_amd.agents.tree_search.state_aware.StateAwarePlannerAgent"),
    ("rl_agents.agents.robust.robust.DiscreteRobustPlannerAgent", "rl_agents_amd.agents.robust.robust.DiscreteRobustPlannerAgent"),
    ("rl_agents.agents.tree_search.mcts_with_prior.MCTSWithPriorPolicyAgent",
     "rl_agents_amd.agents.tree_search.mcts_with_prior.MCTSWithPriorPolicyAgent"),
]
VALUE_ITERATION = [
    ("rl_agents.agents.dynamic_programming.value_iteration.ValueIterationAgent",
     "rl_agents_amd.agents.dynamic_programming.value_iteration.ValueIterationAgent"),
    ("rl_agents.agents.dynamic_programming.robust_value_iteration.RobustValueIterationAgent",
     "rl_agents_amd.agents.dynamic_programming.robust_value_iteration.RobustValueIterationAgent"),
]
AGENT_CONFIG = {"budget": 60, "gamma": 0.75}
TREES = (("uct_highway_small", 5), ("opd_grid_c1", 4))


def klass(path):
    module, name = path.rsplit(".", 1)
    return getattr(importlib.import_module(module), name)


def cls_string(path):
    return "<class '{}'>".format(path)


def factory_record():
    from rl_agents.agents.common.factory import agent_factory, load_agent          # the REFERENCE's factory
    from rl_agents_amd.envs import FiniteMDPEnv, generators

    def env():
        e = FiniteMDPEnv(generators.gridworld())
        e.reset()
        return e

    rec = dict(agent_config=AGENT_CONFIG, env="rl_agents_amd.envs.generators.gridworld()", agents={}, value_iteration={})
    for ref_path, our_path in AGENTS:
        entry = dict(ours=our_path, default_config=klass(ref_path).default_config())
        if "MCTSWithPrior" not in ref_path:       # (its default prior agent is the reference's torch DQN: not constructible)
            agent = agent_factory(env(), dict(AGENT_CONFIG, __class__=cls_string(ref_path)))
            entry.update(config=agent.config, planner_config=agent.planner.config, seed_3=agent.seed(3))
            with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
                json.dump(dict(AGENT_CONFIG, __class__=cls_string(our_path)), f)
            ours = load_agent(f.name, env())
            os.unlink(f.name)
            assert type(ours) is klass(our_path), (our_path, type(ours))
        rec["agents"][ref_path] = entry
    for ref_path, our_path in VALUE_ITERATION:
        rec["value_iteration"][ref_path] = dict(ours=our_path, default_config=klass(ref_path).default_config())
    return rec


def tree_plot_record():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    from rl_agents.agents.tree_search.graphics import TreePlot as RefTreePlot          # the REFERENCE's plot
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_tree_tools import rebuild
    z = np.load(os.path.join(GOLDEN, "tree_tools.npz"))
    rec = dict(max_depth=6, trees={})
    for name, n_actions in TREES:
        planner = types.SimpleNamespace(root=rebuild(z, name),
                                        env=types.SimpleNamespace(action_space=types.SimpleNamespace(n=n_actions)))
        fig, ax = plt.subplots()
        RefTreePlot(planner, max_depth=rec["max_depth"]).plot(filename=None, ax=ax)
        segments = sorted([round(float(ln.get_xdata()[0]), 9), round(float(ln.get_ydata()[0]), 9), round(float(ln.get_xdata()[1]), 9),
                           round(float(ln.get_ydata()[1]), 9), round(float(ln.get_linewidth()), 9)] for ln in ax.lines)
        plt.close(fig)
        rec["trees"][name] = dict(n_actions=n_actions, segments=segments)
    return rec


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_golden_dropin.py <reference checkout>")
    sys.path[:0] = [os.path.join(HERE, "stubs"), os.path.abspath(sys.argv[1]), REPO]
    for name, rec in (("reference_factory.json", factory_record()), ("reference_tree_plot.json", tree_plot_record())):
        with open(os.path.join(GOLDEN, name), "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", os.path.join(GOLDEN, name))


if __name__ == "__main__":
    main()
