"""GBOP, the graph-based optimistic planner for stochastic MDPs (reference
``rl_agents/agents/tree_search/graph_based_stochastic.py``), under the reference's module path and class names.

``StochasticGraphBasedPlanner``, ``StochasticGraphBasedPlannerAgent``, ``GraphDecisionNode``, ``GraphChanceNode`` and
``build_graph`` live in ``rl_agents_amd/gbop.py`` and are served from here by name, so that the reference's ``"__class__"`` line
loads with only its package prefix changed (the way ``mdp_gape`` serves ``StochasticMDPGapEAgent``)."""
_NAMES = ("StochasticGraphBasedPlanner", "StochasticGraphBasedPlannerAgent", "GraphDecisionNode", "GraphChanceNode", "build_graph",
          "ThresholdTables", "PLACEHOLDERS_MESSAGE", "REWARD_THRESHOLD_MESSAGE")


def __getattr__(name):
    if name in _NAMES:
        from rl_agents_amd import gbop
        return getattr(gbop, name)
    raise AttributeError("module {!r} has no attribute {!r}".format(__name__, name))


def __dir__():
    return sorted(set(globals()) | set(_NAMES))
