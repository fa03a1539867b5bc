"""The rows PerEpisodeEvaluation uploads for a ValueIterationAgent prior (boltzmann_prior_rows), by bits, on listing orders that
are not their own inverse: against the unmodified reference's rows (tests/golden/per_episode_order.npz) restricted with the
reference's own formula, and against this package's sequential agents' own steps (ValueIterationAgent.policy_table, then
MCTSWithPriorPolicyAgent.policy_tables).  No GPU: Q tables come from the golden or from a numpy value iteration.

A row summed over permuted columns differs from the row summed in action-id order in the last bits, unless the permutation only
swaps the first two columns -- highway's order, the only one the loops were tested with.  The test asserts of its own inputs
that the two summation orders differ on them: otherwise it could not tell the implementations apart."""
import os

import numpy as np
import pytest

from tests import order_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "per_episode_order.npz")
E, T_STEPS = 4, 3


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(order_cases.ORDERS))
def test_orders_differ_from_their_inverse_and_are_no_adjacent_swap(name):
    order_cases.assert_general_order(order_cases.ORDERS[name])
    available = order_cases.available_of(name)
    assert available.any(axis=1).all()
    assert available.all() == (name == "a8_full")
    with pytest.raises(AssertionError):
        order_cases.assert_general_order((1, 0, 2, 3, 4))           # highway's


def _columns_first(q_dev, temperature, available_dev):
    """The other summation order: exp and the row sum over the DEVICE columns (what the fast path did before)."""
    from rl_agents_amd.trainer.per_episode_evaluation import restrict_and_renormalise
    zz = np.exp((q_dev - q_dev.max(axis=-1, keepdims=True)) / temperature)
    return restrict_and_renormalise(zz / zz.sum(axis=-1, keepdims=True), available_dev)


def _rows_differ(a, b):
    return int((a.view(np.uint64) != b.view(np.uint64)).any(axis=-1).sum())


def _solve(tab, gamma, iterations):
    """value_iteration.py:42-73 on a deterministic table, in numpy."""
    q = np.zeros(tab["reward"].shape)
    for _ in range(iterations):
        nxt = q.max(axis=-1)[tab["transition"]]
        nxt[np.asarray(tab["terminal"]).astype(bool)] = 0
        nxt = tab["reward"] + gamma * nxt
        if np.allclose(q, nxt):
            break
        q = nxt
    return q


@pytest.mark.parametrize("name", ["a3", "a5"])
def test_uploaded_rows_equal_the_reference_rows_of_the_golden(z, name):
    """Every (episode, step) of the golden: the reference prior agent's own Q table, in device columns as vi_solve_batch returns
    it -> the uploaded rows == the reference's Boltzmann rows, permuted and restricted as agent_policy_available does (np.sum
    over the listed actions, in listing order)."""
    from rl_agents_amd.trainer.per_episode_evaluation import boltzmann_prior_rows
    order = [int(a) for a in z[name + "/order"]]
    order_cases.assert_general_order(order)
    assert tuple(order) == order_cases.ORDERS[name]
    available = z[name + "/available"].astype(bool)
    temperature = float(z["prior/temperature"])
    q_dev, want = [], []
    for e in range(E):
        p = "{}/prior/e{}".format(name, e)
        for t in range(len(z[p + "/states"])):
            q_dev.append(z[p + "/q"][t][:, order])
            want.append(order_cases.reference_rows(z[p + "/prior_table"][t], order, available))
    q_dev, want = np.ascontiguousarray(np.stack(q_dev)), np.stack(want)
    got = boltzmann_prior_rows(q_dev, order, temperature, available[:, order])
    assert _rows_differ(_columns_first(q_dev, temperature, available[:, order]).reshape(-1, len(order)),
                        want.reshape(-1, len(order))) > 0, "the inputs cannot tell the two summation orders apart"
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


class _SolvedPrior(object):
    """ValueIterationAgent's own policy_table over a Q table solved elsewhere (its solve is a device call)."""
    finite_mdp = True

    def __init__(self, q, temperature):
        self.state_action_value, self.config = q, {"temperature": temperature}

    def policy_table(self):
        from rl_agents_amd.agents.dynamic_programming.value_iteration import ValueIterationAgent
        return ValueIterationAgent.policy_table(self)


class _Sequential(object):
    """MCTSWithPriorPolicyAgent.policy_tables' own permute-and-restrict steps around that prior."""

    def __init__(self, prior_agent):
        self.prior_agent, self._tables = prior_agent, {}

    def rows(self, model):
        from rl_agents_amd.agents.tree_search.mcts_with_prior import MCTSWithPriorPolicyAgent
        return MCTSWithPriorPolicyAgent.policy_tables(self, None, model)[0]


class _Model(object):
    def __init__(self, s, a, order, available_dev):
        self.S, self.A, self.action_order, self.available = s, a, np.asarray(order, dtype=np.int64), available_dev


@pytest.mark.parametrize("temperature", [0.3, 6.0])
@pytest.mark.parametrize("name", sorted(order_cases.ORDERS))
def test_uploaded_rows_equal_the_sequential_agents_rows(name, temperature):
    """Twelve tables per fixture (four episodes, three steps): the batch's rows == ValueIterationAgent.policy_table() followed by
    MCTSWithPriorPolicyAgent.policy_tables' [:, order] and restriction, table by table."""
    from rl_agents_amd.trainer.per_episode_evaluation import boltzmann_prior_rows
    order = order_cases.ORDERS[name]
    order_cases.assert_general_order(order)
    available_dev = order_cases.available_of(name)[:, list(order)]
    s, a = available_dev.shape
    qs = [_solve(order_cases.table(name, e, t), 0.9, 100) for e in range(E) for t in range(T_STEPS)]
    want = np.stack([_Sequential(_SolvedPrior(q, temperature)).rows(_Model(s, a, order, available_dev)) for q in qs])
    q_dev = np.ascontiguousarray(np.stack(qs)[:, :, list(order)])
    got = boltzmann_prior_rows(q_dev, order, temperature, available_dev)
    assert _rows_differ(_columns_first(q_dev, temperature, available_dev).reshape(-1, a), want.reshape(-1, a)) > 0, \
        "the inputs cannot tell the two summation orders apart"
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_ascending_order_and_no_restriction_are_the_plain_softmax():
    from rl_agents_amd.trainer.per_episode_evaluation import boltzmann_prior_rows
    q = _solve(order_cases.table("a5", 0, 0), 0.9, 100)
    want = _SolvedPrior(q, 0.7).policy_table()
    assert boltzmann_prior_rows(q[None], None, 0.7, None)[0].tobytes() == want.tobytes()
