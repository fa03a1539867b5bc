"""Environments whose finite MDP CHANGES AT EVERY STEP -- the surface of highway-v0, whose ``to_finite_mdp()`` rebuilds the
time-to-collision table from the current traffic each time it is asked (real ``highway_env`` is absent from this image).
Agents of the reference re-read the table at every step (dynamic_programming/value_iteration.py:29-35); a batch of such
episodes is what ``rl_agents_amd.trainer.per_episode_evaluation`` advances with one launch per step."""
import copy

import numpy as np

from . import generators
from .finite_mdp import _TABLE_TOKENS, FiniteMDPEnv, MaskedFiniteMDPEnv, OrderedMaskedFiniteMDPEnv
from .highway_like import HighwayLikeEnv


class _ScheduledTables(object):
    """Tables replaced before every step from a schedule ``tables[t]`` (dicts with transition / reward / terminal; the last one
    stays) -- what a re-extraction does to the env's MDP: new tables, same current state."""

    def __init__(self, tables, state=0, max_steps=0):
        self.tables = [dict(t) for t in tables]
        cfg = {k: v for k, v in self.tables[0].items() if k != "original_shape"}
        cfg.update(state=int(state), max_steps=int(max_steps))
        super(_ScheduledTables, self).__init__(cfg)
        self.reset()

    def _install(self, t):
        tab = self.tables[min(int(t), len(self.tables) - 1)]
        self.mdp.transition = np.ascontiguousarray(tab["transition"], dtype=np.int64)
        self.mdp.reward = np.ascontiguousarray(tab["reward"], dtype=np.float64)
        self.mdp.terminal = np.asarray(tab["terminal"]).astype(bool)

    def reset(self, **kw):
        out = super(_ScheduledTables, self).reset(**kw)
        self._install(0)
        return out

    def step(self, action):
        out = super(_ScheduledTables, self).step(action)
        self._install(self.steps)
        return out


class ScheduledTableEnv(_ScheduledTables, FiniteMDPEnv):
    """A FiniteMDPEnv whose tables follow a schedule (see :class:`_ScheduledTables`)."""


class MaskedScheduledTableEnv(_ScheduledTables, MaskedFiniteMDPEnv):
    """The same over a :class:`MaskedFiniteMDPEnv`: ``tables[0]["available"]`` ([S][A] flags) restricts the action sets of
    every step (``get_available_actions``), as a grid of one shape does."""


class OrderedMaskedScheduledTableEnv(_ScheduledTables, OrderedMaskedFiniteMDPEnv):
    """The same over an :class:`OrderedMaskedFiniteMDPEnv`: ``tables[0]["available"]`` and ``tables[0]["listing_order"]`` (a
    permutation of the action ids) hold for every step; the restriction and the order live on the env object, as on highway."""


class ScheduledModelsEnv(ScheduledTableEnv):
    """A :class:`ScheduledTableEnv` whose schedule holds M tables per step, ``tables[t][m]``: the true environment follows table
    0, and :meth:`hypothesis` hands out the candidate models a discrete robust agent plans on (agents/robust/robust.py:68-71),
    ``config["models"] = [[{"method": "hypothesis", "args": [m]}] for m in range(M)]``."""

    def __init__(self, tables, state=0, max_steps=0):
        self.model_tables = [[dict(tab) for tab in step] for step in tables]
        super(ScheduledModelsEnv, self).__init__([step[0] for step in self.model_tables], state=state, max_steps=max_steps)

    def hypothesis(self, m):
        """A finite-MDP environment in the current state (and step count) holding table ``m`` of the current step.  Its MDP's
        ``tables_version`` names the (step, m) table: asking again for a table that did not change promises identical tables."""
        m = int(m[0] if isinstance(m, (list, tuple)) else m)
        tab = self.model_tables[min(int(self.steps), len(self.model_tables) - 1)][m]
        cfg = {k: v for k, v in tab.items() if k not in ("original_shape", "_version_token")}
        cfg.setdefault("mode", "deterministic")
        cfg.update(state=int(self.mdp.state), max_steps=int(self.config.get("max_steps", 0) or 0))
        env = FiniteMDPEnv(cfg)
        env.mdp.state, env.steps = int(self.mdp.state), int(self.steps)
        token = tab.get("_version_token")
        if token is None:
            token = tab["_version_token"] = next(_TABLE_TOKENS)
        d = env.mdp.__dict__          # (a new object per call over the same table: the table's identity, as HighwayLikeEnv.to_finite_mdp)
        d["_tables_token"], d["_tables_counter"], d["_dirty_log"], d["_dirty_base"], d["_token_shared"] = token, 0, {}, 0, True
        d.pop("_private", None)
        return env


class ChangingHighwayEnv(HighwayLikeEnv):
    """A :class:`HighwayLikeEnv` (restricted action sets listed IDLE first, restriction on the env object) whose table is
    re-drawn after every step: ``highway_shaped(V, L, T, seed = table_seed + steps)``."""

    def __init__(self, n_speeds=3, n_lanes=4, n_times=10, table_seed=0, state=0, collision_rate=0.05):
        self.grid, self.table_seed, self.collision_rate = (n_speeds, n_lanes, n_times), int(table_seed), float(collision_rate)
        super(ChangingHighwayEnv, self).__init__(n_speeds, n_lanes, n_times, state=state, table=self._table(0))

    def _table(self, t):
        return generators.highway_shaped(*self.grid, collision_rate=self.collision_rate, seed=self.table_seed + int(t))

    def reset(self, **kw):
        out = super(ChangingHighwayEnv, self).reset(**kw)
        self.table = self._table(0)
        return out

    def step(self, action):
        out = super(ChangingHighwayEnv, self).step(action)
        self.table = self._table(self.steps)
        return out

    def with_collision_rate(self, rate):
        """A candidate model of this environment: the same table generator at another collision rate, in the current state and
        time (a preprocessor for ``DiscreteRobustPlannerAgent``'s ``config["models"]``)."""
        new = copy.deepcopy(self)
        new.collision_rate = float(rate[0] if isinstance(rate, (list, tuple)) else rate)
        new.table = new._table(new.steps)
        return new
