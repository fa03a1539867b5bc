"""mp_last_kernel_ms after UCT plans (csrc/uct.hip uct_pipeline; csrc/api.hip kernels_begin / kernels_end).

Two events on the ctx stream bracket the launches of a plan call: the one launch of a device-array plan, or the chunks a host-array
call spreads over side streams.  Whatever takes the time (profiles/uct_step_fixed_costs.md measured the events' own packets as
nothing, and the launch that carries its events as no gain), the contract is: the call reports the launches it made and a time
that is its own -- above zero, within the wall time of the call, fresh after every plan."""
import time

import numpy as np
import pytest

from tests.helpers import assert_form

pytestmark = pytest.mark.gpu

K, N_STATES, HORIZON = 5, 40, 8
KNOBS = ("MP_UCT_MODEL", "MP_UCT_QUAD", "MP_UCT_LONE", "MP_UCT_ROWS", "MP_UCT_PATH", "MP_UCT_TREE_STORES", "MP_PIPE_CHUNK", "MP_PIPE_STREAMS")


@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(ctx):
    from rl_agents_amd.envs import generators
    cfg = generators.random_deterministic(N_STATES, K, 7, terminal_rate=0.05)
    m = ctx.load_table(cfg["transition"], cfg["reward"], cfg["terminal"])
    yield m
    m.close()


@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MP_UCT_MODEL", "ldsr")
    return monkeypatch


class DevicePlan:
    """the arrays of a device-array plan of n roots, on the device once"""

    def __init__(self, n):
        import torch
        from rl_agents_amd import native
        dev = torch.device("cuda", 0)
        self.n = n
        self.s0 = torch.from_numpy((np.arange(n) * 3 % N_STATES).astype(np.int32)).to(dev)
        self.rng = torch.from_numpy(native.seed_sequence_states((), 41000, n).view(np.int64)).to(dev)
        self.plans = torch.empty((n, HORIZON), dtype=torch.int32, device=dev)
        self.steps = torch.empty(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def plan(self, ctx, model, episodes):
        """one plan between two synchronisations of the ctx -> (kernel ms, launches, wall ms of the call and its work)"""
        p = np.ones(K) / K
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.uct_plan_device(model, self.n, self.s0, episodes, HORIZON, 0.9, 5.0, p, p, self.rng, HORIZON, plans=self.plans,
                            env_steps=self.steps)
        ctx.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        ms, launches = ctx.last_kernel_ms()
        return ms, launches, wall


def test_device_plan_is_one_launch_timed_within_the_call(ctx, model, knobs):
    d = DevicePlan(4096 + 70)
    d.plan(ctx, model, 33)                                       # (the first launch loads the code object)
    ms, launches, wall = d.plan(ctx, model, 33)
    assert_form(ctx, "uct_ldsr")
    assert launches == 1
    assert 0.0 < ms <= wall, (ms, wall)
    assert int(d.steps.sum().item()) > 0


def test_second_plan_gives_a_fresh_value(ctx, model, knobs):
    d = DevicePlan(4096 + 70)
    d.plan(ctx, model, 2)
    small, n0, _ = d.plan(ctx, model, 2)
    big, n1, wall = d.plan(ctx, model, 400)                      # 200 times the episodes: a time of its own, well above the first
    again, n2, _ = d.plan(ctx, model, 2)
    assert (n0, n1, n2) == (1, 1, 1)
    assert 0.0 < small < big <= wall and 0.0 < again < big, (small, big, again, wall)
    # asking twice without a plan in between reads the same pair of events
    assert ctx.last_kernel_ms() == ctx.last_kernel_ms()


def test_chunked_host_plan_counts_its_chunks(ctx, model, knobs):
    from rl_agents_amd import native
    n = 2 * 1024 + 52
    s0 = (np.arange(n) * 3 % N_STATES).astype(np.int32)
    p = np.ones(K) / K
    knobs.setenv("MP_PIPE_CHUNK", "1024")
    ctx.synchronize()
    t0 = time.perf_counter()
    out = ctx.uct_plan(model, s0, 33, HORIZON, 0.9, 5.0, p, p, native.seed_sequence_states((), 42000, n), max_plan_len=HORIZON)
    wall = 1e3 * (time.perf_counter() - t0)                      # (a host-array call synchronises before it returns)
    assert_form(ctx, "uct_ldsr")
    ms, launches = ctx.last_kernel_ms()
    assert launches == 3
    assert 0.0 < ms <= wall, (ms, wall)
    # the same roots as one chunk: one launch again, the same results
    knobs.setenv("MP_PIPE_CHUNK", "0")
    one = ctx.uct_plan(model, s0, 33, HORIZON, 0.9, 5.0, p, p, native.seed_sequence_states((), 42000, n), max_plan_len=HORIZON)
    ms1, launches1 = ctx.last_kernel_ms()
    assert launches1 == 1 and ms1 > 0.0
    for f in ("plans", "plan_len", "root_value", "env_steps"):
        assert np.array_equal(out[f], one[f]), f
