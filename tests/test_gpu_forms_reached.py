"""Every kernel form the library can record (mp_kernel_form_names) is reached by a test that asserts its name.

FORMS maps every name of OPD, robust OPD, state-aware OPD and UCT on stochastic models to the smallest shape and the knobs that
select it; test_form_is_reached runs that plan on 1 to 70 roots, asserts the recorded name and compares with the oracle exactly
as the planner's own tests do -- status, plans, bounds or values, env steps, generator records, and the whole tree of two roots,
all on bits.  ELSEWHERE points the names of UCT, batched VI, OLOP, BRUE and GBOP-D at the tests that assert them.
test_table_covers_every_form (no GPU) holds the two tables to the library's list: no omissions, no skip list.
test_saopd_form_is_the_one_the_host_query_names holds mp_saopd_choose_form (tests/test_saopd_forms.py pins it without a GPU) to
what the state-aware plans of both tables record.

EDGES are the thresholds the choices turn on, each with the case on its other side:
  stochastic UCT   sparse rows of width 2 whose rewards take exactly 256 distinct bit patterns, +0.0 and -0.0 among them
                   (compact records, r1) and 257 (r2); dense rows whose fullest holds 2, 4, 5 non-zeros (r2 / r1, r4, r0);
                   1 + episodes |A| = 65 535 nodes (16-bit path entries) and 65 537 (32-bit), on trees that fill them
  OPD, robust OPD  |A| = 2: budget 43, the last where the compact closing pass fits the bounds array, and 44;
                   the wide kernel's row at 128 slots and the next step up (sibling layout; residue classes: 127 and 129)
  state-aware OPD  S = 117, the last with 16 depth entries beside the LDS dictionaries, and 118; a kept planner planned until
                   its arena leaves LDS (budget 1200 on the 10 x 10 grid: the fourth plan); a call that rolls back
                   (MP_SAOPD_QUEUE); the sorted dispatch order on a second plan"""
import numpy as np
import pytest

from tests.helpers import assert_form, bfs_by_parent, opd_closing_fits

STOCH_RECORDS = (0, 2, 4, 1)
STOCH_ACTIONS = ("any", 2, 3, 4, 5, 6, 7, 8)


# ---- the table -----------------------------------------------------------------------------------------------------------------
def opd_case(n_actions, budget, knobs="", models=0, terminal_reward=0.25, n_roots=5):
    return dict(planner="ropd" if models else "opd", n_actions=n_actions, budget=budget, knobs=knobs, models=models,
                terminal_reward=terminal_reward, n_roots=n_roots)


def opd_forms():
    """|A| = 4, budget 100 wherever a knob selects the form; |A| = 2 at budget 44 where the closing pass leaves the compact
    tables by itself; |A| = 64 at the budgets around a row of 128 slots for the wide kernel's two instantiations."""
    forms = {"opd_any": opd_case(65, 195, n_roots=70), "ropd_any": opd_case(65, 195, models=2, n_roots=70)}
    for x, model in (("lds", "MP_OPD_MODEL=lds"), ("ldsx", "MP_OPD_MODEL=ldsx")):
        forms["opd_" + x] = opd_case(4, 100, model, n_roots=70)
        forms["opd_{}_chain".format(x)] = opd_case(2, 44, model)
        forms["opd_{}_gen".format(x)] = opd_case(4, 100, model + " MP_OPD_LOOP=0")
        forms["opd_{}_gen_chain".format(x)] = opd_case(2, 44, model, terminal_reward=-0.5)
        for loop, m, knob in (("m2", 2, ""), ("m4", 3, ""), ("gen", 5, "")):
            forms["ropd_{}_{}".format(x, loop)] = opd_case(4, 100, model + knob, models=m, n_roots=70 if m == 2 else 5)
            forms["ropd_{}_{}_chain".format(x, loop)] = opd_case(2, 44, model + knob, models=m)
    for layout, wide, small, big in (("sib", "", 8128, 8192), ("cls", " MP_OPD_WIDE=cls", 8064, 8128)):
        knobs = "MP_OPD_MODEL=global" + wide
        forms["opd_wide_{}_small".format(layout)] = opd_case(4, 100, knobs, n_roots=70)
        forms["opd_wide_{}_small_gen".format(layout)] = opd_case(64, small, knobs, terminal_reward=-0.5, n_roots=2)
        forms["opd_wide_" + layout] = opd_case(64, big, knobs, n_roots=2)
        forms["opd_wide_{}_gen".format(layout)] = opd_case(64, big, knobs + " MP_OPD_LOOP=0", n_roots=2)
        forms["ropd_wide_" + layout] = opd_case(4, 100, knobs, models=2, n_roots=70)
        forms["ropd_wide_{}_gen".format(layout)] = opd_case(4, 100, knobs, models=2, terminal_reward=-0.5)
    return forms


def saopd_case(names, model="grid", knobs="", budgets=None, n=5, warm=False):
    """``names``: the form of every plan of the episode, the last one being the table's; ``warm``: an earlier batch has planned
    on the model (fresh planners then have costs to sort by)."""
    return dict(planner="saopd", names=names, model=model, knobs=knobs, budgets=budgets or [120] * len(names), n=n, warm=warm)


def saopd_forms():
    """The 10 x 10 grid (budget 120) for every form a knob selects; "decay" is the three-state table of zero rewards whose
    values decay to underflow (tests/test_gpu_batch.py): tens of thousands of backups fill a queue of 256 entries."""
    plain = "MP_SAOPD_DICT=0 MP_SAOPD_LDS=0"
    return {
        "saopd_lane": saopd_case(["saopd_lane"], knobs="MP_SAOPD_MODEL=lane", n=70),
        "saopd_lane_retry": saopd_case(["saopd_lane_retry"], "decay", "MP_SAOPD_MODEL=lane MP_SAOPD_QUEUE=256"),
        "saopd_wave": saopd_case(["saopd_wave"], knobs=plain, n=70),
        "saopd_wave_retry": saopd_case(["saopd_wave_retry"], "decay", plain + " MP_SAOPD_QUEUE=256"),
        "saopd_wave_ordered": saopd_case(["saopd_wave", "saopd_wave_ordered"], knobs=plain + " MP_SAOPD_ORDER=1"),
        "saopd_wave_ordered_retry": saopd_case(["saopd_wave_ordered_retry"], "decay", plain + " MP_SAOPD_ORDER=1 MP_SAOPD_QUEUE=256",
                                               warm=True),
        "saopd_wave_dict": saopd_case(["saopd_wave_dict"], n=70),
        # the all-in-LDS form is asked for: its queue of 256 entries fills, and so does the next form's
        "saopd_wave_dict_retry": saopd_case(["saopd_wave_dict_retry"], "decay", "MP_SAOPD_LDS=1 MP_SAOPD_QUEUE=256"),
        "saopd_wave_dict_ordered": saopd_case(["saopd_wave_dict", "saopd_wave_dict_ordered"], knobs="MP_SAOPD_ORDER=1"),
        "saopd_wave_dict_ordered_retry": saopd_case(["saopd_wave_dict_ordered_retry"], "decay", "MP_SAOPD_ORDER=1 MP_SAOPD_QUEUE=256",
                                                    warm=True),
        "saopd_wave_lds": saopd_case(["saopd_wave_lds"], knobs="MP_SAOPD_LDS=1", n=70),
        "saopd_wave_lds_ordered": saopd_case(["saopd_wave_lds", "saopd_wave_lds_ordered"], knobs="MP_SAOPD_LDS=1 MP_SAOPD_ORDER=1"),
    }


def stoch_case(records, bits, actions, policy, rows=None, episodes=None, horizon=None, n_roots=None, closed=None, knobs="",
               temperature=4.5):
    """``rows``: the model (stoch_model); the defaults give the smallest plan with that many path-entry bits."""
    a = 9 if actions == "any" else actions
    closed = (a % 2 == 1) if closed is None else closed
    if rows is None:
        rows = {0: "sparse5" if policy else "dense", 2: "sparse2", 4: "sparse3", 1: "sparse2-few"}[records]
    if episodes is None:        # 32 bits: the first plan whose 1 + episodes (|A| + closed) node slots pass 65 535
        episodes = 20 if bits == 16 or policy else -(-65535 // (a + closed))
    wide = bits == 32 and not policy
    return dict(planner="stoch", records=records, bits=bits, n_actions=a, policy=policy, rows=rows, episodes=episodes,
                horizon=horizon or (3 if wide else 5), n_roots=n_roots or (2 if wide else 70), closed=closed, knobs=knobs,
                temperature=temperature)


def stoch_name(records, bits, actions, policy=False):
    return "uct_stoch_r{}_p{}_a{}{}".format(records, bits, actions, "_policy" if policy else "")


def stoch_forms():
    forms = {}
    for r in STOCH_RECORDS:
        for a in STOCH_ACTIONS:
            forms[stoch_name(r, 16, a)] = stoch_case(r, 16, a, False)
            forms[stoch_name(r, 32, a)] = stoch_case(r, 32, a, False)
            forms[stoch_name(r, 32, a, True)] = stoch_case(r, 32, a, True)
    return forms


FORMS = {}
FORMS.update(opd_forms())
FORMS.update(saopd_forms())
FORMS.update(stoch_forms())

# the planners whose tests asserted their forms before this table existed: name -> the test that asserts it
ELSEWHERE = {
    "uct_global": "tests/test_gpu_batch.py::test_uct_batch_highway_headline_shape",
    "uct_global_spill": "tests/test_gpu_batch.py::test_uct_long_horizons_spill_the_path_stack",
    "uct_ldsr": "tests/test_gpu_batch.py::test_uct_batch_highway_headline_shape",
    "uct_quad": "tests/test_gpu_uct_quad.py::test_quad_headline_geometry",
    "uct_lone": "tests/test_gpu_uct_lone.py::test_lone_headline_geometry",
    "uct_lone_mw": "tests/test_gpu_uct_lone.py::test_lone_multi_wave_headline_geometry",
    "uct_lone_each": "tests/test_gpu_forged_draws.py::test_uct_tie_draws_one_model_per_root",
    "uct_row_each": "tests/test_gpu_forged_draws.py::test_uct_tie_draws_one_model_per_root",
    "uct_row_shared": "tests/test_gpu_uct_rows.py::test_rows_headline_geometry_default",
    "uct_cartpole": "tests/test_gpu_cartpole.py::test_cartpole_every_replication_factor_vs_oracle",
    "uct_policy": "tests/test_gpu_forged_draws.py::test_uct_listed_policies_first_draws_on_every_threshold",
    "vi_batch_reg<1,64>": "tests/test_gpu_per_episode.py::test_vi_batch_register_forms",
    "vi_batch_reg<2,64>": "tests/test_gpu_per_episode.py::test_vi_batch_register_forms",
    "vi_batch_reg<2,128>": "tests/test_gpu_per_episode.py::test_vi_batch_register_forms",
    "vi_batch_reg<2,256>": "tests/test_gpu_per_episode.py::test_vi_batch_register_forms",
    "vi_batch_reg<4,256>": "tests/test_gpu_per_episode.py::test_vi_batch_register_forms",
    "vi_batch_reg<4,512>": "tests/test_gpu_per_episode.py::test_vi_batch_register_forms",
    "vi_batch_reg<4,1024>": "tests/test_gpu_per_episode.py::test_vi_batch_register_forms",
    "vi_batch_cluster2": "tests/test_gpu_per_episode.py::test_vi_batch_cluster_small_mdps_and_fallback",
    "vi_batch_cluster4": "tests/test_gpu_per_episode.py::test_vi_batch_cluster_form",
    "vi_batch_cluster8": "tests/test_gpu_per_episode.py::test_vi_batch_cluster_form",
    "vi_batch_wg_stream": "tests/test_gpu_per_episode.py::test_vi_batch_workgroup_forms",
    "vi_batch_wg_lds": "tests/test_gpu_per_episode.py::test_vi_batch_workgroup_forms",
    "vi_batch_wg_global": "tests/test_gpu_per_episode.py::test_vi_batch_workgroup_forms",
    "olop_global": "tests/test_gpu_olop.py::test_batches_against_the_restatement",
    "olop_global_slots": "tests/test_gpu_olop.py::test_batches_against_the_restatement",
    "brue_global": "tests/test_gpu_forged_draws.py::test_brue_action_draws",
    "brue_global_slots": "tests/test_gpu_brue.py::test_wide_nodes_and_workgroup_slots",
    "gbopd_wave_lds": "tests/test_gpu_gbopd.py::test_ten_thousand_states_from_global_memory",
    "gbopd_wave_global": "tests/test_gpu_gbopd.py::test_ten_thousand_states_from_global_memory",
}

# the node-count edges: a temperature at which the prior term of the selection rule outweighs every value, so that the tree grows
# in breadth and no descent reaches the horizon before it has expanded a node
DEEP_H, DEEP_T = 24, 1e6

# ---- the thresholds: (id, the form on this side, the case) ---------------------------------------------------------------------
EDGES = [
    ("rewards-256", "uct_stoch_r1_p16_a3", stoch_case(1, 16, 3, False, rows="sparse2-256")),
    ("rewards-257", "uct_stoch_r2_p16_a3", stoch_case(2, 16, 3, False, rows="sparse2-257")),
    ("dense-row-2", "uct_stoch_r2_p16_a4", stoch_case(2, 16, 4, False, rows="dense-2")),
    ("dense-row-2-few-rewards", "uct_stoch_r1_p16_a4", stoch_case(1, 16, 4, False, rows="dense-2-few")),
    ("dense-row-4", "uct_stoch_r4_p16_a4", stoch_case(4, 16, 4, False, rows="dense-4")),
    ("dense-row-5", "uct_stoch_r0_p16_a4", stoch_case(0, 16, 4, False, rows="dense-5")),
    ("unfused", "uct_stoch_r0_p16_a3", stoch_case(0, 16, 3, False, rows="sparse2-few", knobs="MP_UCT_STOCH_FUSED=0")),
    ("kept-at-32-bytes", "uct_stoch_r2_p16_a3", stoch_case(2, 16, 3, False, rows="sparse2-few", knobs="MP_UCT_STOCH_FUSED=2")),
    ("loop-form-forced", "uct_stoch_r2_p16_aany", stoch_case(2, 16, 5, False, knobs="MP_UCT_STOCH_GENERIC_A=1")),
    ("nodes-65535", "uct_stoch_r2_p16_a2", stoch_case(2, 16, 2, False, rows="sparse2-deep", episodes=32767, horizon=DEEP_H, n_roots=1,
                                                      closed=False, temperature=DEEP_T)),
    ("nodes-65537", "uct_stoch_r2_p32_a2", stoch_case(2, 32, 2, False, rows="sparse2-deep", episodes=32768, horizon=DEEP_H, n_roots=1,
                                                      closed=False, temperature=DEEP_T)),
    ("closing-fits", "opd_lds", opd_case(2, 43)),
    ("closing-fits-not", "opd_lds_chain", opd_case(2, 44)),
    ("closing-fits", "ropd_lds_m2", opd_case(2, 43, models=2)),
    ("closing-fits-not", "ropd_lds_m2_chain", opd_case(2, 44, models=2)),
    ("row-128", "opd_wide_sib_small", opd_case(64, 8128, "MP_OPD_MODEL=global", n_roots=2)),
    ("row-192", "opd_wide_sib", opd_case(64, 8192, "MP_OPD_MODEL=global", n_roots=2)),
    ("row-127", "opd_wide_cls_small", opd_case(64, 8064, "MP_OPD_MODEL=global MP_OPD_WIDE=cls", n_roots=2)),
    ("row-129", "opd_wide_cls", opd_case(64, 8128, "MP_OPD_MODEL=global MP_OPD_WIDE=cls", n_roots=2)),
    ("row-128", "ropd_wide_sib", opd_case(64, 8128, "MP_OPD_MODEL=global", models=2, n_roots=2)),
    ("row-192", "ropd_wide_sib", opd_case(64, 8192, "MP_OPD_MODEL=global", models=2, n_roots=2)),
    ("dict-117-states", "saopd_wave_dict", saopd_case(["saopd_wave_dict"], "garnet117", "MP_SAOPD_LDS=0")),
    ("dict-118-states", "saopd_wave", saopd_case(["saopd_wave"], "garnet118", "MP_SAOPD_LDS=0")),
    ("dict-118-states-default", "saopd_wave_lds", saopd_case(["saopd_wave_lds"], "garnet118")),
    ("asked-for-beyond-117-states", "saopd_wave", saopd_case(["saopd_wave"], "garnet118", "MP_SAOPD_DICT=1 MP_SAOPD_LDS=0")),
    ("leaves-lds", "saopd_wave_dict", saopd_case(["saopd_wave_lds"] * 3 + ["saopd_wave_dict"], knobs="MP_SAOPD_LDS=1", budgets=[1200] * 4,
                                                 n=3)),
    ("no-costs-yet", "saopd_wave_dict", saopd_case(["saopd_wave_dict"], knobs="MP_SAOPD_ORDER=1")),
    ("costs-of-an-earlier-batch", "saopd_wave_dict_ordered", saopd_case(["saopd_wave_dict_ordered"], knobs="MP_SAOPD_ORDER=1", warm=True)),
    ("rolls-back-a-kept-planner", "saopd_wave_dict_retry",
     saopd_case(["saopd_wave_lds", "saopd_wave_dict_retry"], "decay", "MP_SAOPD_QUEUE=256", budgets=[8, 120])),
]

KNOBS = ("MP_OPD_MODEL", "MP_OPD_WIDE", "MP_OPD_CLOSING", "MP_OPD_LOOP", "MP_SAOPD_MODEL", "MP_SAOPD_LDS", "MP_SAOPD_DICT",
         "MP_SAOPD_ORDER", "MP_SAOPD_QUEUE", "MP_UCT_STOCH_FUSED", "MP_UCT_STOCH_GENERIC_A")


# ---- without a GPU -------------------------------------------------------------------------------------------------------------
def test_table_covers_every_form():
    """FORMS and ELSEWHERE together name exactly what the library can record; every pointer names a test that exists and whose
    file spells the form (or the format that builds it)."""
    import os
    import re
    from rl_agents_amd import native
    names = native.kernel_form_names()
    assert len(names) == len(set(names)) and all(len(n) < 48 for n in names)
    assert not set(FORMS) & set(ELSEWHERE)
    assert set(FORMS) | set(ELSEWHERE) == set(names), sorted((set(FORMS) | set(ELSEWHERE)) ^ set(names))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, where in ELSEWHERE.items():
        path, test = where.split("::")
        text = open(os.path.join(repo, path)).read()
        assert re.search(r"^def {}\(".format(test), text, re.M), where
        stem = re.sub(r"(<.*|\d+)$", "", name)
        assert stem in text, (name, where)
    for name, case in FORMS.items():
        assert case["planner"] == name.split("_")[0].replace("uct", "stoch"), name
    for _, name, case in EDGES:
        assert name in FORMS and case["planner"] == FORMS[name]["planner"], name


def test_edge_budgets_are_the_thresholds():
    """The budgets of the closing-pass edges: 44 is the first at which the compact tables do not fit |A| = 2."""
    assert all(opd_closing_fits(2, b) for b in range(0, 44)) and not opd_closing_fits(2, 44)
    assert opd_closing_fits(4, 100) and opd_closing_fits(64, 8192) and opd_closing_fits(65, 195)


# ---- on the device -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from rl_agents_amd import native
    c = native.Context(0)
    yield c
    c.close()


def records(g, n):
    r = g.integers(0, 2 ** 63, size=(n, 6), dtype=np.int64).astype(np.uint64)
    r[:, 3] |= np.uint64(1)
    r[:, 4:] = 0
    return r


def run_opd(ctx, name, case):
    from oracle import oracle
    from rl_agents_amd.envs import generators
    a, budget, n, m, tr = case["n_actions"], case["budget"], case["n_roots"], case["models"], case["terminal_reward"]
    cfg = generators.random_deterministic(60, a, seed=500 + a, terminal_rate=0.05)
    g = np.random.Generator(np.random.PCG64(budget))
    s0 = g.integers(0, 60, size=n).astype(np.int32)
    rng = records(g, n)
    rng0, rng_ref = rng.copy(), rng.copy()
    mpl, cap = budget // a + 2, 1 + (budget // a) * a
    if m:
        others = [generators.rewire(cfg, 0.15, seed=10 + i) for i in range(m - 1)]
        t = np.stack([cfg["transition"]] + [o["transition"] for o in others])
        r = np.stack([cfg["reward"]] + [o["reward"] for o in others])
        term = np.stack([cfg["terminal"]] + [o["terminal"] for o in others])
        model = ctx.load_joint(t, r, term)
        roots = np.repeat(s0[:, None], m, axis=1)
        out = ctx.ropd_plan(model, s0, budget, 0.9, tr, rng, max_plan_len=mpl)
        assert_form(ctx, name)
        ref = oracle.ropd_plan_batch(t, r, term, roots, budget, 0.9, tr, rng_ref, max_plan_len=mpl)
    else:
        t, r, term = cfg["transition"], cfg["reward"], cfg["terminal"]
        model = ctx.load_table(t, r, term)
        out = ctx.opd_plan(model, s0, budget, 0.9, tr, rng, max_plan_len=mpl)
        assert_form(ctx, name)
        ref = oracle.opd_plan_batch(t, r, term, s0, budget, 0.9, tr, rng_ref, max_plan_len=mpl)
    for k in ("status", "plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.array_equal(out["root_lower"], ref["root_lower"]) and np.array_equal(out["root_upper"], ref["root_upper"])
    np.testing.assert_array_equal(rng, ref["rng_after"])
    assert (out["status"] == 0).any()
    for root in sorted({0, n - 1}):
        if out["status"][root] != 0:
            continue
        if m:
            tree = ctx.ropd_tree(root, cap, m)
            one = oracle.ropd_plan(t, r, term, roots[root], budget, 0.9, tr, rng0[root].copy(), max_plan_len=mpl)["tree"]
        else:
            tree = ctx.opd_tree(root, cap)
            one = oracle.opd_plan(t, r, term, int(s0[root]), budget, 0.9, tr, rng0[root].copy(), max_plan_len=mpl)["tree"]
        for k in one:
            np.testing.assert_array_equal(tree[k], one[k], err_msg="tree[{}] of root {}".format(k, root))
    model.close()


def saopd_model(kind):
    from rl_agents_amd.envs import generators
    if kind == "grid":
        cfg = generators.gridworld()
    elif kind == "decay":
        r = np.zeros((3, 4))
        r[2, 1] = 0.25
        return np.array([[0, 2, 2, 1], [1, 1, 2, 2], [1, 1, 0, 1]]), r, np.zeros(3, bool), 0.9
    else:
        cfg = generators.random_deterministic(int(kind[6:]), 4, seed=7)
    return cfg["transition"], cfg["reward"], cfg["terminal"], 0.8


def run_saopd(ctx, name, case):
    from oracle import oracle
    from rl_agents_amd import native
    assert case["names"][-1] == name
    t, r, term, gamma = saopd_model(case["model"])
    n = case["n"]
    model = ctx.load_table(t, r, term)
    g = np.random.Generator(np.random.PCG64(len(name)))
    states = g.integers(0, r.shape[0], size=n).astype(np.int32)
    rng = records(g, n)
    if case["warm"]:
        warm = native.StateAwarePlanners(ctx, model, n)
        warm.plan(states[::-1].copy(), case["budgets"][0], gamma, 0.0, rng.copy())
        warm.close()
    planners = native.StateAwarePlanners(ctx, model, n)
    ref_rng, ref_planner, dead = rng.copy(), [None] * n, np.zeros(n, bool)
    for step, (budget, form) in enumerate(zip(case["budgets"], case["names"])):
        out = planners.plan(states, budget, gamma, 0.0, rng, max_plan_len=budget + 1)
        assert_form(ctx, form)
        for i in range(n):
            if dead[i]:
                continue
            try:
                o = oracle.saopd_plan(t, r, term, int(states[i]), budget, gamma, rng_state=ref_rng[i], planner=ref_planner[i],
                                      max_plan_len=budget + 1)
            except ValueError:
                assert out["status"][i] == native.MP_ERR_ARG, (step, i)
                dead[i] = True
                continue
            assert out["status"][i] == 0, (step, i)
            np.testing.assert_array_equal(out["plans"][i, :out["plan_len"][i]], o["plan"], err_msg=str((step, i)))
            assert out["env_steps"][i] == o["env_steps"] and out["updates"][i] == o["updates"], (step, i)
            np.testing.assert_array_equal(rng[i], o["rng_after"])
            ref_rng[i], ref_planner[i] = o["rng_after"], o["planner"]
            if i in (0, n - 1):
                tree, sv = planners.export(i)
                assert np.array_equal(sv, o["state_values"]), (step, i)
                for k in ("parent", "first_child", "state", "depth", "lower", "reward", "alive", "count"):
                    assert np.array_equal(tree[k], o["tree"][k]), (step, i, k)
        states = np.where(out["plan_len"] > 0, t[states, np.maximum(out["plans"][:, 0], 0)], states).astype(np.int32)
    assert not dead.all()
    planners.close()
    model.close()


def few_rewards(shape, patterns):
    """Rewards that take exactly ``patterns`` distinct bit patterns, +0.0 and -0.0 the first two."""
    values = np.concatenate([[0.0, -0.0], np.arange(1, patterns - 1) / 300.0])
    assert len(set(values.view(np.uint64).tolist())) == patterns
    return values[np.arange(int(np.prod(shape))) % patterns].reshape(shape)


def stoch_model(rows, n_actions):
    """-> (mode, transition, next or None, reward, terminal): 130 states, so that two actions make 260 rows -- room for 257
    rewards.  sparseB: B successors per row; "-few": 38 rewards; "-256" / "-257": exactly so many bit patterns; "-deep": no
    terminal state, every episode expands a node; dense-B: full rows of 130 entries whose fullest holds B non-zeros (successors
    listed twice merge, so most rows hold fewer)."""
    from rl_agents_amd.envs import generators
    n_states = 130
    kind, _, tag = rows.partition("-")
    if kind == "dense" and not tag:
        cfg = generators.random_stochastic(30, n_actions, seed=60 + n_actions, terminal_rate=0.05)
        return "stochastic", cfg["transition"], None, cfg["reward"], cfg["terminal"]
    if kind == "dense":
        b = int(tag.split("-")[0])
        sp = generators.random_sparse(n_states, n_actions, b, seed=70 + b, terminal_rate=0.05)
        sp["next"][0, 0] = np.arange(b)         # one row with b distinct successors
        dense = np.zeros((n_states, n_actions, n_states))
        for j in range(b):
            np.add.at(dense, (np.arange(n_states)[:, None], np.arange(n_actions)[None, :], sp["next"][:, :, j]), sp["transition"][:, :, j])
        assert int((dense > 0).sum(axis=2).max()) == b
        reward = np.round(sp["reward"] * 37) / 37 if tag.endswith("few") else sp["reward"]
        return "stochastic", dense, None, reward, sp["terminal"]
    b = int(kind[6:])
    sp = generators.random_sparse(n_states, n_actions, b, seed=80 + b + n_actions, terminal_rate=0.0 if tag == "deep" else 0.05)
    reward = sp["reward"]
    if tag == "few":
        reward = np.round(reward * 37) / 37
    elif tag in ("256", "257"):
        reward = few_rewards(reward.shape, int(tag))
    else:
        assert len(np.unique(reward)) > 256
    return "sparse", sp["transition"], sp["next"], reward, sp["terminal"]


def stoch_inputs(case):
    """Everything run_stoch hands to the device and the oracle, from the case alone."""
    a, n = case["n_actions"], case["n_roots"]
    mode, p, nxt, reward, term = stoch_model(case["rows"], a)
    g = np.random.Generator(np.random.PCG64(1000 * case["records"] + 10 * a + case["bits"]))
    s0 = g.integers(0, reward.shape[0], size=n).astype(np.int32)
    rng, erng = records(g, n), records(g, n)
    if case["policy"]:
        prior = g.random(reward.shape) + 0.1
        prior /= prior.sum(axis=1, keepdims=True)
        roll = g.random(reward.shape) + 0.1
        roll /= roll.sum(axis=1, keepdims=True)
    else:
        prior = g.random(a) + 0.1
        prior /= prior.sum()
        roll = g.random(a) + 0.1
        roll /= roll.sum()
    return mode, p, nxt, reward, term, s0, rng, erng, prior, roll


def stoch_reference(case, inputs, root):
    from oracle import oracle
    mode, p, nxt, reward, term, s0, rng, erng, prior, roll = inputs
    mpl = (2 if case["closed"] else 1) * case["horizon"]
    return oracle.uct_plan_stoch(mode, p, reward, term, int(s0[root]), case["episodes"], case["horizon"], 0.9, case["temperature"], prior, roll,
                                 rng[root].copy(), erng[root], next_states=nxt, closed_loop=case["closed"], max_plan_len=mpl)


def test_the_deep_trees_fill_the_node_slots():
    """(No GPU.)  The oracle's trees of the two node-count edges hold every slot the plan has room for: node ids up to 65 534
    reach the 16-bit path entries, 65 536 the 32-bit ones."""
    for _, _, case in EDGES:
        if case.get("rows") == "sparse2-deep":
            tree = stoch_reference(case, stoch_inputs(case), 0)["tree"]
            assert len(tree["parent"]) == 1 + 2 * case["episodes"] > 65000


def run_stoch(ctx, name, case):
    from oracle import oracle
    inputs = stoch_inputs(case)
    mode, p, nxt, reward, term, s0, rng0, erng, prior, roll = inputs
    rng, closed, n = rng0.copy(), case["closed"], case["n_roots"]
    model = ctx.load_sparse(p, nxt, reward, term) if mode == "sparse" else ctx.load_dense(p, reward, term)
    policy = ctx.load_policy(model, prior, roll) if case["policy"] else None
    mpl = (2 if closed else 1) * case["horizon"]
    out = ctx.uct_plan_stochastic(model, s0, case["episodes"], case["horizon"], 0.9, case["temperature"], None if policy else prior,
                                  None if policy else roll, rng, env_rng_state=erng, closed_loop=closed, max_plan_len=mpl, policy=policy)
    assert_form(ctx, name)
    ref = oracle.uct_plan_stoch_batch(mode, p, reward, term, s0, case["episodes"], case["horizon"], 0.9, case["temperature"], prior, roll, rng0.copy(),
                                      erng, next_states=nxt, closed_loop=closed, max_plan_len=mpl, n_threads=8)
    for k in ("plans", "plan_len", "env_steps"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.array_equal(out["root_value"], ref["root_value"])
    np.testing.assert_array_equal(rng, ref["rng_after"])
    for root in sorted({0, n - 1}):
        tree, one = ctx.uct_stoch_tree(root), stoch_reference(case, inputs, root)["tree"]
        (oa, pa), (ob, pb) = bfs_by_parent(tree["parent"]), bfs_by_parent(one["parent"])
        np.testing.assert_array_equal(pa, pb)
        for k in ("action", "is_obs", "count", "value"):
            assert np.array_equal(np.asarray(tree[k])[oa], np.asarray(one[k])[ob]), (root, k)
    if policy is not None:
        policy.close()
    model.close()


RUN = {"opd": run_opd, "ropd": run_opd, "saopd": run_saopd, "stoch": run_stoch}


def run_case(ctx, monkeypatch, name, case):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in case["knobs"].split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv(k, v)
    RUN[case["planner"]](ctx, name, case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FORMS))
def test_form_is_reached(ctx, monkeypatch, name):
    run_case(ctx, monkeypatch, name, FORMS[name])


@pytest.mark.gpu
@pytest.mark.parametrize("edge", range(len(EDGES)), ids=["{}-{}".format(n, e) for e, n, _ in EDGES])
def test_form_at_the_threshold(ctx, monkeypatch, edge):
    _, name, case = EDGES[edge]
    run_case(ctx, monkeypatch, name, case)


SAOPD_CASES = [(name, case) for name, case in sorted(FORMS.items()) if case["planner"] == "saopd"] + \
              [(edge, case) for edge, _, case in EDGES if case["planner"] == "saopd"]


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(SAOPD_CASES)), ids=[w for w, _ in SAOPD_CASES])
def test_saopd_form_is_the_one_the_host_query_names(ctx, monkeypatch, which):
    """Before every plan of every state-aware case above, mp_saopd_choose_form is asked about the call from what a caller knows
    -- the sizes, the rows mp_saopd_info reports, whether there are costs to sort by, host arrays; not the rows and queue entries
    allocated -- and names what the plan then records: the first launch, or, where the call rolled back, the fallback."""
    from rl_agents_amd import native
    case = SAOPD_CASES[which][1]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in case["knobs"].split():
        k, v = kv.split("=", 1)
        monkeypatch.setenv(k, v)
    t, r, term, gamma = saopd_model(case["model"])
    n, cus = case["n"], ctx.device_info()["n_cu"]
    model = ctx.load_table(t, r, term)
    g = np.random.Generator(np.random.PCG64(len(case["names"][-1])))
    states = g.integers(0, r.shape[0], size=n).astype(np.int32)
    rng = records(g, n)
    if case["warm"]:
        warm = native.StateAwarePlanners(ctx, model, n)
        warm.plan(states[::-1].copy(), case["budgets"][0], gamma, 0.0, rng.copy())
        warm.close()
    planners = native.StateAwarePlanners(ctx, model, n)
    for step, (budget, form) in enumerate(zip(case["budgets"], case["names"])):
        have_cost = case["warm"] or step > 0
        first, fallback, _ = native.saopd_choose_form([n, r.shape[0], r.shape[1], budget, planners.info()["n_nodes"], 0, 0, have_cost, 0, cus])
        out = planners.plan(states, budget, gamma, 0.0, rng, max_plan_len=budget + 1)
        recorded = ctx.last_kernel_variant()
        assert recorded == form, (step, recorded)
        assert "_retry" not in first and "_retry" not in fallback
        if recorded.endswith("_retry"):
            assert fallback == recorded[:-len("_retry")], (step, first, fallback, recorded)
        else:
            assert first == recorded, (step, first, fallback, recorded)
        states = np.where(out["plan_len"] > 0, t[states, np.maximum(out["plans"][:, 0], 0)], states).astype(np.int32)
    planners.close()
    model.close()
