"""The host side of mp_uct_plan* and mp_uct_plan_stochastic* (csrc/uct_host.hpp and the table of the caller's arrays): two ways
of making the same call give the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OUTPUTS = ("plans", "plan_len", "root_value", "root_child_count", "root_child_value", "env_steps")


@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chunk_case(ctx):
    """2049 roots = two whole chunks of 1024 and a ragged one of a single root; every root starts at a step count of its own
    and the model's max_steps cuts the rollouts of those that start late (horizon 7, at most 9 - root_steps steps left)."""
    from rl_agents_amd import native
    from rl_agents_amd.envs import generators
    cfg = generators.highway_shaped(4, 5, 12, seed=21)
    t, r, term = cfg["transition"], cfg["reward"], cfg["terminal"]
    model = ctx.load_table(t, r, term, max_steps=9)
    n = 2049
    g = np.random.Generator(np.random.PCG64(21))
    roots = g.choice(np.flatnonzero(~term), size=n).astype(np.int32)
    steps = (1 + np.arange(n) % 6).astype(np.int32)
    prior = g.random((model.S, model.A)) + 0.1
    prior /= prior.sum(axis=1, keepdims=True)
    roll = g.random((model.S, model.A)) + 0.1
    roll /= roll.sum(axis=1, keepdims=True)
    policy = ctx.load_policy(model, prior, roll)
    yield dict(model=model, n=n, roots=roots, steps=steps, rng0=native.seed_sequence_states([21], 0, n), policy=policy,
               prior_p=prior[0].copy(), rollout_p=roll[1].copy())
    policy.close()
    model.close()


@pytest.mark.parametrize("per_state", [True, False], ids=["policy", "plain"])
def test_chunked_call_with_every_optional_array_equals_the_single_launch(ctx, chunk_case, per_state, monkeypatch):
    """mp_uct_plan / mp_uct_plan_policy on pageable arrays, root_steps given and all six results asked for: the call in chunks
    of 1024 roots on two streams (3 launches) leaves the results, the generator records and the trees of the roots at the
    chunk edges exactly as the single launch does.  The plain case again with only plan_len and env_steps asked for, in pinned
    buffers, and generator records resident on the device: root_steps is still a pageable array, so the call copies by chunk."""
    c = chunk_case
    model, n = c["model"], c["n"]
    kw = dict(root_steps=c["steps"], max_plan_len=7, policy=c["policy"] if per_state else None)
    args = (6, 7, 0.8, 10.0, None, None) if per_state else (6, 7, 0.8, 10.0, c["prior_p"], c["rollout_p"])
    probe = (0, 1023, 1024, 2048)
    monkeypatch.setenv("MP_PIPE_STREAMS", "2")
    monkeypatch.setenv("MP_PIPE_CHUNK", "0")
    ctx.uct_reset_tree()
    rng_a = c["rng0"].copy()
    ref = ctx.uct_plan(model, c["roots"], *args, rng_a, **kw)
    assert ctx.last_kernel_ms()[1] == 1
    assert set(ref) == set(OUTPUTS)
    assert (ref["env_steps"] < 6 * 7).any() and len(set(ref["env_steps"].tolist())) > 1, "max_steps is meant to cut some rollouts"
    trees_ref = [ctx.uct_tree(i) for i in probe]
    monkeypatch.setenv("MP_PIPE_CHUNK", "1024")
    rng_b = c["rng0"].copy()
    out = ctx.uct_plan(model, c["roots"], *args, rng_b, **kw)
    assert ctx.last_kernel_ms()[1] == 3
    for k in OUTPUTS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(rng_b, rng_a)
    for i, tr in zip(probe, trees_ref):
        got = ctx.uct_tree(i)
        for k in tr:
            np.testing.assert_array_equal(got[k], tr[k], err_msg="tree of root {} / {}".format(i, k))
    if per_state:
        return
    bufs = ctx.plan_buffers(n, 7, outputs=("plan_len", "env_steps"))
    bufs["root_state"][:] = c["roots"]
    dev_rng = ctx.device_rng(c["rng0"])
    out2 = ctx.uct_plan(model, bufs["root_state"], *args, dev_rng, root_steps=c["steps"], out=bufs)
    assert ctx.last_kernel_ms()[1] == 3
    assert set(out2) == {"root_state", "plan_len", "env_steps"}
    for k in ("plan_len", "env_steps"):
        np.testing.assert_array_equal(out2[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(dev_rng.get(), rng_a)
    dev_rng.close()
    bufs.close()


def _stoch_plan(ctx, model, a, closed, mem, skip=()):
    """mp_uct_plan_stochastic on the arrays of `a` (numpy arrays or device tensors), the results named in `skip` passed as NULL."""
    from rl_agents_amd import native
    p = {k: (None if k in skip else native._ptr(v)) for k, v in a.items()}
    n = int(a["root_state"].shape[0])
    native._check(ctx._lib.mp_uct_plan_stochastic(
        ctx._h, model._h, n, p["root_state"], p["root_steps"], 8, 5, 0.9, 3.0, native._ptr(a["prior_p"]), native._ptr(a["rollout_p"]),
        int(closed), p["rng"], p["env_rng"], int(a["plans"].shape[1]), p["plans"], p["plan_len"], p["root_value"],
        p["root_child_count"], p["root_child_value"], p["env_steps"], mem))


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
@pytest.mark.parametrize("mode", ["sparse", "stochastic"])
def test_stochastic_call_through_every_memory_flavour(ctx, mode, closed):
    """mp_uct_plan_stochastic with root_steps and the env's generator records on 130 roots (two whole wavefronts and a ragged
    third): pageable arrays (staged through the workspaces), mp_host_alloc arrays (read and written in place) and device tensors
    give the same results, generator records and trees; a result left out (NULL) leaves the other five as they are."""
    import torch
    from rl_agents_amd import native
    from rl_agents_amd.envs import generators
    if mode == "sparse":
        cfg = generators.random_sparse(40, 3, 2, seed=7, terminal_rate=0.05)
        model = ctx.load_sparse(cfg["transition"], cfg["next"], cfg["reward"], cfg["terminal"])
    else:
        cfg = generators.random_stochastic(40, 3, seed=7, terminal_rate=0.05)
        model = ctx.load_dense(cfg["transition"], cfg["reward"], cfg["terminal"])
    model.set_episode_rules("source", 7)
    n, mpl = 130, 10 if closed else 5
    g = np.random.Generator(np.random.PCG64(7))
    s0 = g.integers(0, 40, size=n).astype(np.int32)
    steps0 = g.integers(0, 5, size=n).astype(np.int32)
    rng0, erng = native.seed_sequence_states([7], 0, n), native.seed_sequence_states([8], 0, n)
    prior, roll = np.array([0.5, 0.2, 0.3]), np.array([0.25, 0.35, 0.4])
    probe = (0, 63, 64, 129)

    # pageable numpy arrays
    rng_a = rng0.copy()
    ref = ctx.uct_plan_stochastic(model, s0, 8, 5, 0.9, 3.0, prior, roll, rng_a, env_rng_state=erng, closed_loop=closed,
                                  root_steps=steps0)
    assert not np.array_equal(rng_a, rng0)
    trees_ref = [ctx.uct_stoch_tree(i) for i in probe]

    def same_trees(what):
        for i, tr in zip(probe, trees_ref):
            got = ctx.uct_stoch_tree(i)
            for k in tr:
                np.testing.assert_array_equal(got[k], tr[k], err_msg="{}: tree of root {} / {}".format(what, i, k))

    # every array in pinned memory
    pin = ctx.pinned(dict(root_state=((n,), np.int32), root_steps=((n,), np.int32), rng=((n, 6), np.uint64),
                          env_rng=((n, 6), np.uint64), plans=((n, mpl), np.int32), plan_len=((n,), np.int32),
                          root_value=((n,), np.float64), root_child_count=((n, 3), np.int64),
                          root_child_value=((n, 3), np.float64), env_steps=((n,), np.int64)))
    a = dict(pin, prior_p=prior, rollout_p=roll)
    a["root_state"][:], a["root_steps"][:], a["rng"][:], a["env_rng"][:], a["plans"][:] = s0, steps0, rng0, erng, -1
    _stoch_plan(ctx, model, a, closed, native.MP_MEM_HOST)
    for k in OUTPUTS:
        np.testing.assert_array_equal(a[k], ref[k], err_msg="pinned " + k)
    np.testing.assert_array_equal(a["rng"], rng_a)
    np.testing.assert_array_equal(a["env_rng"], erng)
    same_trees("pinned")
    del a
    pin.close()

    # device tensors
    def dev(x):
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).cuda()
    d = dict(root_state=dev(s0), root_steps=dev(steps0), rng=dev(rng0.copy()), env_rng=dev(erng),
             plans=dev(np.full((n, mpl), -1, np.int32)), plan_len=dev(np.zeros(n, np.int32)), root_value=dev(np.zeros(n)),
             env_steps=dev(np.zeros(n, np.int64)))
    torch.cuda.synchronize()
    ctx.uct_plan_stochastic_device(model, n, d["root_state"], 8, 5, 0.9, 3.0, prior, roll, d["rng"], d["env_rng"], mpl,
                                   closed_loop=closed, plans=d["plans"], plan_len=d["plan_len"], root_value=d["root_value"],
                                   env_steps=d["env_steps"], root_steps=d["root_steps"])
    ctx.synchronize()
    for k in ("plans", "plan_len", "root_value", "env_steps"):
        np.testing.assert_array_equal(d[k].cpu().numpy(), ref[k], err_msg="device " + k)
    np.testing.assert_array_equal(d["rng"].cpu().numpy().view(np.uint64), rng_a)
    same_trees("device")

    # host arrays, one result left out
    h = dict(root_state=s0, root_steps=steps0, rng=rng0.copy(), env_rng=erng, prior_p=prior, rollout_p=roll,
             plans=np.full((n, mpl), -1, np.int32), plan_len=np.zeros(n, np.int32), root_value=np.zeros(n),
             root_child_count=np.zeros((n, 3), np.int64), root_child_value=np.full((n, 3), -7.0), env_steps=np.zeros(n, np.int64))
    _stoch_plan(ctx, model, h, closed, native.MP_MEM_HOST, skip=("root_child_value",))
    for k in OUTPUTS:
        if k != "root_child_value":
            np.testing.assert_array_equal(h[k], ref[k], err_msg="without root_child_value: " + k)
    assert (h["root_child_value"] == -7.0).all()
    np.testing.assert_array_equal(h["rng"], rng_a)
    model.close()
