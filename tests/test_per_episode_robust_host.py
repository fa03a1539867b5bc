"""The discrete robust planner with one set of M models per episode, host side: tests/golden/per_episode_robust.npz (the
UNMODIFIED reference DiscreteRobustPlanner, one object per episode, on model sets replaced before every step) against the CPU
oracle, so that fixture and oracle vouch for each other and the GPU tests may use the oracle on random cases; the header's new
entry points; ScheduledModelsEnv's hypotheses."""
import os
import re

import numpy as np
import pytest

from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
E, T_STEPS = 6, 3
CONFIGS = ["m2", "m3"]


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(HERE, "golden", "per_episode_robust.npz"))


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", CONFIGS)
def test_oracle_reproduces_the_reference_on_every_episode_and_step(z, name):
    """oracle.ropd_plan on every (episode, step): the plan, both root bounds on bits, the generator record -- continued from step
    to step -- and the env steps of the reference planner."""
    m = int(z[name + "/n_models"])
    budget, gamma, tr = int(z[name + "/budget"]), float(z[name + "/gamma"]), float(z[name + "/terminal_reward"])
    assert z[name + "/transition"].shape[:3] == (E, T_STEPS, m)
    planned = 0
    for e in range(E):
        rng = z["{}/e{}/rng_before".format(name, e)].copy()
        total = 0
        n_steps = int(z["{}/e{}/n_steps".format(name, e)])
        assert n_steps >= 1
        for t in range(n_steps):
            p = "{}/e{}/t{}".format(name, e, t)
            s = int(z["{}/e{}/states".format(name, e)][t])
            res = oracle.ropd_plan(z[name + "/transition"][e, t], z[name + "/reward"][e, t], z[name + "/terminal"][e, t],
                                   np.full(m, s, np.int32), budget, gamma, tr, rng_state=rng, max_plan_len=budget + 1)
            assert res["plan"].tolist() == z[p + "/plan"].tolist(), p
            assert bits(res["root_lower"]) == bits(z[p + "/root_lower"]), p
            assert bits(res["root_upper"]) == bits(z[p + "/root_upper"]), p
            np.testing.assert_array_equal(res["rng_after"], z[p + "/rng_after"], err_msg=p)
            total += int(res["env_steps"])
            assert total == int(z[p + "/env_steps_total"]), p
            rng = res["rng_after"].copy()
            planned += 1
    assert planned > E              # some episode goes beyond its first step: the generator does continue somewhere


def test_fixture_holds_what_the_issue_asks_for(z):
    assert (int(z["m2/n_models"]), int(z["m2/budget"]), float(z["m2/gamma"]), float(z["m2/terminal_reward"])) == (2, 150, 0.8, 0.0)
    assert (int(z["m3/n_models"]), int(z["m3/budget"]), float(z["m3/gamma"]), float(z["m3/terminal_reward"])) == (3, 100, 0.9, 0.5)
    for name in CONFIGS:
        t = z[name + "/transition"]
        assert t.shape[3:] == (120, 5)
        # every step's set differs from the one before, and a hypothesis differs from the true table
        assert all((t[e, k] != t[e, k + 1]).any() for e in range(E) for k in range(T_STEPS - 1))
        assert all((t[e, k, 0] != t[e, k, 1]).any() for e in range(E) for k in range(T_STEPS))
    assert os.path.getsize(os.path.join(HERE, "golden", "per_episode_robust.npz")) < 128 * 1024


def test_header_declares_the_joint_batch_entry_points():
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    for name in ("mp_model_load_joint_batch", "mp_model_update_joint_tables", "mp_model_set_available_joint_batch",
                 "mp_ropd_plan_models"):
        assert re.search(r"\bint\s+{}\s*\(".format(name), header), name
    assert re.search(r"#define\s+MP_ABI_VERSION\s+7\b", header)
    from rl_agents_amd import native
    for name in ("mp_model_load_joint_batch", "mp_model_update_joint_tables", "mp_model_set_available_joint_batch",
                 "mp_ropd_plan_models"):
        assert name in native.SIGNATURES
    # model_index, root_state, then the tail of mp_ropd_plan
    assert native.SIGNATURES["mp_ropd_plan_models"][1][4:] == native.SIGNATURES["mp_ropd_plan"][1][3:]


def test_scheduled_models_env_hands_out_the_current_steps_tables(z):
    from rl_agents_amd import device_model
    from rl_agents_amd.agents.common.factory import preprocess_env
    from rl_agents_amd.envs import ScheduledModelsEnv
    name, e = "m3", 1
    tables = [[dict(mode="deterministic", transition=z[name + "/transition"][e, t, m], reward=z[name + "/reward"][e, t, m],
                    terminal=z[name + "/terminal"][e, t, m]) for m in range(3)] for t in range(T_STEPS)]
    env = ScheduledModelsEnv(tables, state=int(z["s0"][e]))
    env.reset()
    for t in range(T_STEPS + 1):
        k = min(t, T_STEPS - 1)                         # the last set stays
        s = int(env.mdp.state)
        assert np.array_equal(env.mdp.transition, z[name + "/transition"][e, k, 0])     # the true env follows table 0
        versions = []
        for m in range(3):
            h = preprocess_env(env, [{"method": "hypothesis", "args": [m]}])
            mdp = device_model.finite_mdp_of(h)
            assert mdp.mode == "deterministic" and int(mdp.state) == s and h.steps == env.steps
            assert np.array_equal(mdp.transition, z[name + "/transition"][e, k, m])
            assert np.array_equal(mdp.reward, z[name + "/reward"][e, k, m])
            assert np.array_equal(mdp.terminal, z[name + "/terminal"][e, k, m])
            version = mdp.tables_version
            assert isinstance(version, tuple) and version[0] is not None
            assert env.hypothesis(m).mdp.tables_version == version      # the same table again: the same version
            versions.append(version)
            h.step(0)                                   # stepping a hypothesis leaves the true environment alone
            assert int(env.mdp.state) == s
        assert len(set(versions)) == 3
        if t == T_STEPS:
            assert versions == before                   # past the schedule's end nothing changed
        elif t:
            assert not set(versions) & set(before)
        before = versions
        env.step(1)


def test_changing_highway_env_with_collision_rate():
    from rl_agents_amd.envs import ChangingHighwayEnv, generators
    env = ChangingHighwayEnv(3, 4, 10, table_seed=40, state=52, collision_rate=0.05)
    env.reset()
    env.step(1)
    other = env.with_collision_rate(0.15)
    want = generators.highway_shaped(3, 4, 10, collision_rate=0.15, seed=41)
    assert np.array_equal(other.table["transition"], want["transition"]) and np.array_equal(other.table["reward"], want["reward"])
    assert np.array_equal(other.table["terminal"], want["terminal"])
    assert other.state_index == env.state_index and other.steps == env.steps == 1
    assert other.get_available_actions() == env.get_available_actions()
    assert env.collision_rate == 0.05 and env.with_collision_rate([0.15]).collision_rate == 0.15
    other.step(0)
    assert env.steps == 1
