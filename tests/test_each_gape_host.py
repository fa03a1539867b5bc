"""MDP-GapE on one MDP per root (mp_gape_plan_models): what the host decides without a device -- the new symbols, the names of
the forms and mp_gape_each_form_info, the function the launch code itself calls for the form, the LDS bytes and the grid
(rl_agents_amd/csrc/each_host.hpp); the ``kind=`` opt-in of PerEpisodeEvaluation with the recording stand-ins of
tests/test_planner_calls_host.py; the fixture of the unmodified reference (tests/golden/per_episode_gape.npz) against the
restatement the GPU tests compare the device with (tests/gape_restatement.py); and what the per-root sweep of
tests/test_gpu_each_gape.py contains (tests/gape_each_cases.py)."""
import os
import re
import types

import numpy as np
import pytest

from rl_agents_amd import native, runtime
from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
from tests import gape_each_cases as ge
from tests import gape_restatement as gr
from tests.gape_cases import MARGIN, SKIP_CAP
from tests.helpers import generator_from
from tests.test_planner_calls_host import KINDS, UCT, Ctx, Models, plain_env, planner_classes

LDS = 160 * 1024            # bytes of LDS of a compute unit (csrc/common.hpp kLdsBytes): what fits, what the knob can force
DEFAULT = LDS // 16         # kEachLdsDefaultBytes: no table above it takes the LDS form by default
REC = 16                    # bytes of a packed transition record
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "per_episode_gape.npz")
BOUND_TOL = 1e-12
MIN_ROOTS = 256             # kGapeLdsMinRoots: the smallest batch at which the LDS form was measured ahead beyond the spread
AB = os.path.join(HERE, "..", "profiles", "gape_each_ab.json")


def path_bytes(horizon):
    return 16 * -(-4 * (horizon + 1) // 16)


@pytest.fixture
def no_knob(monkeypatch):
    monkeypatch.delenv("MP_EACH_MODEL", raising=False)


def test_symbols_names_and_abi(no_knob):
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+MP_ABI_VERSION\s+7\b", header)
    lib = native.load()
    assert lib.mp_abi_version() == 7
    for symbol in ("mp_gape_plan_models", "mp_gape_each_form_info"):
        assert symbol in native.SIGNATURES and getattr(lib, symbol) is not None, symbol
        declared = re.search(r"\bint %s\(([^;]*)\);" % symbol, header).group(1)
        assert len(native.SIGNATURES[symbol][1]) == declared.count(",") + 1, symbol
    assert re.search(r"\bconst char \*mp_gape_each_form_names\(void\);", header)
    assert "mp_gape_each_form_names" in native.SIGNATURES and lib.mp_gape_each_form_names is not None
    # model_index in front of the roots, the rest mp_gape_plan's in its order
    plain, models = native.SIGNATURES["mp_gape_plan"][1], native.SIGNATURES["mp_gape_plan_models"][1]
    assert list(models) == list(plain[:3]) + [plain[3]] + list(plain[3:])
    names = native.gape_each_form_names()
    assert names == ["gape_each_lds", "gape_each_lds_slots", "gape_each_global", "gape_each_global_slots"]
    others = (native.kernel_form_names(), native.each_form_names(), native.ss_form_names(), native.ss_each_form_names(),
              native.olop_stoch_form_names(), native.gape_form_names(), native.gape_stoch_form_names(), native.vi_form_names())
    for other in others:
        assert not set(names) & set(other)
    # the pinned lists are what they were
    assert len(native.kernel_form_names()) == 172
    assert native.gape_form_names() == ["gape_global", "gape_global_slots"]
    assert native.ss_each_form_names() == ["ss_each_lds", "ss_each_global"]
    assert len(native.each_form_names()) == 8
    assert native.EACH_PLANNERS == {"olop": 0, "brue": 1, "ss": 2}


def test_planner_3_of_the_shared_query_is_still_an_error():
    out = np.zeros(6, np.int64)
    assert native.load().mp_each_form_info(3, 10, 3, 3, 10, 256, out.ctypes.data) == native.MP_ERR_ARG
    with pytest.raises(native.NativeError):
        native.gape_each_form_info(0, 3, 3, 10)
    with pytest.raises(native.NativeError):
        native.gape_each_form_info(10, 3, 0, 10)           # mp_gape_plan_models refuses horizon 0
    with pytest.raises(native.NativeError):
        native.gape_each_form_info(10, 3, 3, 0)


def test_lds_bytes_default_and_grid(no_knob):
    for s_each, a, h, n, cus in [(120, 5, 6, 65536, 256), (120, 5, 6, 7, 256), (6, 2, 2, 1000, 256), (1000, 3, 9, 9000, 256),
                                 (2000, 5, 4, 9000, 104), (12, 70, 16, 3, 256), (30, 140, 70, 5, 256)]:
        info = native.gape_each_form_info(s_each, a, h, n, cus)
        need = path_bytes(h) + s_each * a * REC
        assert info["lds_bytes"] == need and info["default_limit"] == DEFAULT and info["fit_limit"] == LDS
        lds_per_cu = min(32, LDS // need) if need <= LDS else 0
        # the default (profiles/gape_each_ab.json): a footprint that leaves 16 wavefronts to a compute unit, from 256 roots on,
        # and only while every root's workgroup is resident at once
        assert info["lds"] == (need <= DEFAULT and MIN_ROOTS <= n <= cus * lds_per_cu)
        assert info["launch_lds_bytes"] == (need if info["lds"] else path_bytes(h))
        assert info["grid"] == min(n, cus * (lds_per_cu if info["lds"] else 32))
    # never the default above kEachLdsDefaultBytes, whatever was measured below it
    assert native.gape_each_form_info((DEFAULT - 32) // (3 * REC), 3, 6, 1000, 256)["lds"]
    assert not native.gape_each_form_info((DEFAULT - 32) // (3 * REC) + 1, 3, 6, 1000, 256)["lds"]
    # the highway shape: 17 workgroups of the LDS form to a compute unit
    assert [native.gape_each_form_info(120, 5, 6, n, 256)["lds"] for n in (1, 255, 256, 4096, 256 * 17, 256 * 17 + 1, 65536)] == \
        [False, False, True, True, True, False, False]
    # the highway shape at the baseline's horizon 6: 32 bytes of path + 9.6 KB of records
    assert native.gape_each_form_info(120, 5, 6, 4096, 256)["lds_bytes"] == 32 + 9600


def test_knob_and_fit(monkeypatch):
    monkeypatch.setenv("MP_EACH_MODEL", "lds")
    info = native.gape_each_form_info(120, 5, 6, 65536, 256)
    assert info["lds"] and info["grid"] == 256 * (LDS // 9632) == 256 * 17 and info["launch_lds_bytes"] == 9632
    big = native.gape_each_form_info(1000, 3, 3, 65536, 256)            # 48 016 bytes: beyond the default limit, forced
    assert big["lds"] and big["grid"] == 256 * 3
    h = 6
    s_max = (LDS - path_bytes(h)) // (3 * REC)                          # the largest S_each at |A| = 3 that fits, and one more
    fits, over = native.gape_each_form_info(s_max, 3, h, 1000, 256), native.gape_each_form_info(s_max + 1, 3, h, 1000, 256)
    assert fits["lds"] and fits["lds_bytes"] <= LDS and fits["grid"] == 256
    assert not over["lds"] and over["lds_bytes"] > LDS and over["launch_lds_bytes"] == path_bytes(h) and over["grid"] == 1000
    assert native.gape_each_form_info(1, 3, h, 5, 256)["lds"]
    monkeypatch.setenv("MP_EACH_MODEL", "global")
    info = native.gape_each_form_info(120, 5, 6, 256, 256)              # (the default at this batch size is the LDS form)
    assert not info["lds"] and info["grid"] == 256 and info["launch_lds_bytes"] == 32 and info["lds_bytes"] == 9632


def test_the_default_is_what_was_measured(no_knob):
    """profiles/gape_each_ab.json: the LDS form is the default exactly at the batch sizes where it beat the global form by more
    than the spread between repeated medians."""
    import json
    with open(AB) as f:
        rows = [r for r in json.load(f) if r.get("measure") == "forms"]
    assert [r["roots"] for r in rows] == [1, 256, 4096, 65536]
    for r in rows:
        assert (r["S_each"], r["A"], r["horizon"], r["episodes"], r["accuracy"]) == (120, 5, 6, 14, 0.1) and r["bit_identical"]
        info = native.gape_each_form_info(120, 5, 6, r["roots"], 256)
        assert info["lds"] == r["lds_wins_beyond_spread"], r["roots"]


# ---- the opt-in of the per-episode loop ------------------------------------------------------------------------------------------
def evaluation_of(cls, kind=None, **config):
    env = plain_env()
    config = dict(UCT, C=2, **config)
    planner = cls(env, config)
    planner.models = Models(Ctx())
    return PerEpisodeEvaluation([plain_env(), plain_env()], types.SimpleNamespace(planner=planner, config=config), kind=kind)


def test_kind_on_request(monkeypatch):
    monkeypatch.setattr(runtime, "get_context", lambda *a, **k: Ctx.current)
    from rl_agents_amd import gape_stochastic
    classes = planner_classes()
    assert classes["MDPGapE"].per_episode_kind is None and classes["MDPGapE"].per_episode_kind_on_request == "gape"
    assert classes["SparseSampling"].per_episode_kind is None and classes["SparseSampling"].per_episode_kind_on_request == "ss"
    assert gape_stochastic.StochasticMDPGapE.per_episode_kind_on_request is None
    for name, kind in (("MDPGapE", "gape"), ("SparseSampling", "ss")):
        ev = evaluation_of(classes[name], kind=kind)
        assert (ev.kind, ev.subtree, ev.vi) == (kind, False, False)
        # the default is the refusal it was, to the letter
        with pytest.raises(NotImplementedError) as raised:
            evaluation_of(classes[name])
        assert str(raised.value) == str(KINDS[name])
        with pytest.raises(NotImplementedError, match="step_strategy"):
            evaluation_of(classes[name], kind=kind, step_strategy="subtree")
    # a kind a planner declares may be named; another planner's may not
    assert evaluation_of(classes["OLOP"], kind="olop").kind == "olop"
    for cls, kind, offered in ((classes["OLOP"], "gape", "'olop'"), (gape_stochastic.StochasticMDPGapE, "gape", "none"),
                               (classes["MDPGapE"], "olop", "'gape'"), (classes["SparseSampling"], "gape", "'ss'"),
                               (classes["MDPGapE"], "subtree", "'gape'")):
        with pytest.raises(ValueError) as raised:
            evaluation_of(cls, kind=kind)
        assert cls.__name__ in str(raised.value) and offered in str(raised.value)
    with pytest.raises(NotImplementedError):
        evaluation_of(gape_stochastic.StochasticMDPGapE)


def test_planners_have_their_own_plan_call():
    from rl_agents_amd.agents.tree_search.mdp_gape import MDPGapE
    from rl_agents_amd.agents.tree_search.olop import OLOP
    from rl_agents_amd.agents.tree_search.sparse_sampling import SparseSampling
    assert MDPGapE.plan_on is not OLOP.plan_on and MDPGapE.raise_for_result is not OLOP.raise_for_result
    assert "plan_on" in vars(SparseSampling) and "raise_for_result" in vars(SparseSampling)
    calls = []

    class GapeCtx(object):
        def gape_plan(self, model, roots, episodes, horizon, gamma, accuracy, uniform, n_env, column, thr, vin, rng, model_index=None):
            calls.append(dict(n_env=n_env, column=column, thr=len(thr), vin=len(vin), model_index=model_index))
            return dict(status=np.asarray([0, native.ERR_GAPE_NO_CHALLENGER]))

    planner = MDPGapE(plain_env(), dict(UCT))
    planner.models = types.SimpleNamespace(ctx=GapeCtx())
    model = types.SimpleNamespace(A=3, action_order=np.asarray([2, 0, 1]))
    out = planner.plan_on(model, [0, 1], [0, 0], np.zeros((2, 6), np.uint64), model_index=[1, 0], max_plan_len=1)
    assert calls[0]["n_env"] == 3 and calls[0]["column"].tolist() == [1, 2, 0] and calls[0]["model_index"] == [1, 0]
    assert calls[0]["thr"] == UCT["episodes"] + 2 and calls[0]["vin"] == UCT["horizon"] + 1
    with pytest.raises(ValueError, match="empty sequence"):
        planner.raise_for_result(out)
    # the stochastic planner's plan call is its own, and it is the other kernel's
    from rl_agents_amd.gape_stochastic import PLACEHOLDERS_MESSAGE, StochasticMDPGapE
    assert "plan_on" in vars(StochasticMDPGapE) and StochasticMDPGapE.plan_on is not MDPGapE.plan_on
    assert "raise_for_result" in vars(StochasticMDPGapE) and "plan_batch" in vars(StochasticMDPGapE)

    class GapeStochCtx(object):
        def gape_plan_stochastic(self, model, roots, episodes, horizon, count, gamma, accuracy, uniform, n_env, column, thr, tthr,
                                 vin, rng):
            calls.append(dict(count=count, n_env=n_env, column=column, thr=len(thr), tthr=len(tthr), vin=len(vin)))
            return dict(status=np.asarray([0, native.ERR_GAPE_PLACEHOLDERS, native.ERR_GAPE_NO_CHALLENGER]))

    planner = StochasticMDPGapE(plain_env(), dict(UCT, max_next_states_count=2))
    planner.models = types.SimpleNamespace(ctx=GapeStochCtx())          # (no gape_plan: the inherited call would fail here)
    out = planner.plan_on(model, [0, 1, 2], [0, 0, 0], np.zeros((3, 6), np.uint64))
    assert calls[1] == dict(count=2, n_env=3, column=calls[1]["column"], thr=UCT["episodes"] + 2, tthr=UCT["episodes"] + 2,
                            vin=UCT["horizon"] + 1) and calls[1]["column"].tolist() == [1, 2, 0]
    with pytest.raises(ValueError) as raised:
        planner.raise_for_result(out)
    assert str(raised.value) == PLACEHOLDERS_MESSAGE
    with pytest.raises(ValueError, match="empty sequence"):
        planner.raise_for_result(dict(status=out["status"][::-1]))
    with pytest.raises(NotImplementedError, match="one model per episode"):
        planner.plan_on(model, [0], [0], np.zeros((1, 6), np.uint64), model_index=[0])
    assert len(calls) == 2


# ---- the fixture of the unmodified reference against the restatement -------------------------------------------------------------
def fixture_case(z, name, e, t):
    n_actions = z["reward"].shape[-1]
    return dict({"mdp/" + k: z[k][e, t] for k in ("transition", "reward", "terminal")},
                available=np.ones(z["reward"].shape[-2:], bool), order=np.arange(n_actions), done_on_next=False,
                **{k: z["{}/{}".format(name, k)] for k in ("horizon", "episodes", "gamma", "accuracy", "confidence", "continuation",
                                                            "threshold")})


def test_the_fixture_equals_the_restatement_step_by_step():
    """Every discrete output of the unmodified reference's per-episode agents, and the bounds of the root's arms and of the stored
    tree within 1e-12 / (1 - gamma): this pins the fixture and the restatement to each other without a GPU."""
    from tests.test_gape_host import case_thresholds
    z = np.load(GOLDEN)
    assert [str(n) for n in z["configs"]] == ["baseline", "full"]
    assert (int(z["baseline/horizon"]), int(z["baseline/episodes"]), float(z["baseline/gamma"]), float(z["baseline/accuracy"])) == \
        (6, 14, 0.8, 0.1) and str(z["baseline/threshold"]) == "1*np.log(time)"
    assert (z["reward"] >= 1e-3).all() and (z["reward"] <= 1 - 1e-3).all()
    n, trees = len(z["s0"]), 0
    assert n == 7
    for name in ("baseline", "full"):
        gamma = float(z[name + "/gamma"])
        lengths, draws = [], []
        for e in range(n):
            steps = int(z["{}/e{}/n_steps".format(name, e)])
            lengths.append(steps)
            assert int(z["{}/e{}/states".format(name, e)][0]) == int(z["s0"][e])
            record = None
            for t in range(steps):
                p = "{}/e{}/t{}".format(name, e, t)
                if record is not None:
                    np.testing.assert_array_equal(record, z[p + "/rng_before"], err_msg=p)   # the stream runs on from plan to plan
                assert float(z[p + "/margin"]) > MARGIN, p
                case = fixture_case(z, name, e, t)
                gen = generator_from(z[p + "/rng_before"])
                res = gr.gape_plan(case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"],
                                   int(z["{}/e{}/states".format(name, e)][t]), int(case["episodes"]), int(case["horizon"]), gamma,
                                   float(case["accuracy"]), case_thresholds(case), str(case["continuation"]), gen)
                record = native.rng_state_from_generator(gen)
                assert res["error"] is None and res["plan"].tolist() == z[p + "/plan"].tolist(), p
                np.testing.assert_array_equal(record, z[p + "/rng_after"], err_msg=p)
                assert res["episodes_run"] == int(z[p + "/episodes_run"]) and res["env_steps"] == int(z[p + "/env_steps"]), p
                arms = np.flatnonzero((res["kind"] == 1) & (res["parent"] == 0))
                assert res["action"][arms].tolist() == z[p + "/arm_action"].tolist(), p
                assert res["count"][arms].tolist() == z[p + "/arm_count"].tolist(), p
                for mine, theirs in (("vl", "arm_lower"), ("vu", "arm_upper")):
                    assert np.all(np.abs(res[mine][arms] - z[p + "/" + theirs]) <= BOUND_TOL / (1 - gamma)), (p, mine)
                draws.append(int(z[p + "/tie_draws"]))
                if p + "/tree/parent" in z.files:
                    tree = gr.as_bfs(res)
                    for k in ("parent", "kind", "action", "depth", "count", "done", "cum"):
                        assert np.array_equal(tree[k], z[p + "/tree/" + k]), (p, k)
                    for k in ("mu_ucb", "mu_lcb", "vu", "vl"):
                        assert np.all(np.abs(tree[k] - z[p + "/tree/" + k]) <= BOUND_TOL / (1 - gamma)), (p, k)
                    trees += 1
        # an episode that ends by its own actions and the tie draws are in the fixture
        assert lengths[0] == 2 and max(lengths) == 3 and min(draws) >= 1, name
    assert trees == 2
    assert os.path.getsize(GOLDEN) < 256 * 1024


# ---- the per-root sweep ----------------------------------------------------------------------------------------------------------
def test_the_sweep_stays_within_its_cap_and_holds_what_it_is_for():
    left_out, plans, widths, horizons, masked = 0, 0, set(), set(), 0
    for i in range(ge.N_CASES):
        case = ge.each_case(i)
        n_states, n_actions = case["base"]["mdp/reward"].shape
        widths.add(n_actions)
        horizons.add(int(case["base"]["horizon"]))
        masked += case["masked"]
        if case["masked"]:          # every table lists other actions: a form that reads another table's flags is caught
            assert len({c["available"].tobytes() for c in case["tables"]}) == ge.TABLES
        assert len({c["mdp/transition"].tobytes() for c in case["tables"]}) == ge.TABLES
        for c in case["tables"]:
            assert (c["mdp/reward"] >= 1e-3).all() and (c["mdp/reward"] <= 1 - 1e-3).all()
        for res, _, margin in ge.restate_each(case):
            plans += 1
            left_out += not margin > MARGIN
    assert plans == 120
    print("per-root sweep: {} of {} plans have a margin <= {}".format(left_out, plans, MARGIN))
    assert left_out <= SKIP_CAP * plans
    assert {80, 103, 127, 140} <= widths and max(horizons) == 70 and masked == 8
    # the wide tables pass the default limit of the LDS form and fit a compute unit's LDS: forced, they take it
    sizes = sorted(c["base"]["mdp/reward"].size * REC for c in (ge.each_case(i) for i in range(5, ge.N_CASES, 6)))
    assert DEFAULT < sizes[-1] <= LDS - path_bytes(70)
