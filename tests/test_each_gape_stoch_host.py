"""MDP-GapE with transition bounds on one MDP per root (mp_gape_plan_stochastic_models): what the host decides without a device --
the new symbols, the names of the forms and mp_gape_stoch_each_form_info, the function the launch code itself calls for the form,
the LDS bytes and the grid (rl_agents_amd/csrc/each_host.hpp); the planner's call with a ``model_index`` and the ``kind=`` opt-in
of PerEpisodeEvaluation under the planner's per-episode name; the fixture of the unmodified reference
(tests/golden/per_episode_gape_stoch.npz) against the restatement the GPU tests compare the device with
(tests/gape_stoch_restatement.py); and what the per-root sweep of tests/test_gpu_each_gape_stoch.py contains
(tests/gape_stoch_each_cases.py)."""
import os
import re
import types

import numpy as np
import pytest

from rl_agents_amd import native, runtime
from rl_agents_amd.trainer.per_episode_evaluation import PerEpisodeEvaluation
from tests import gape_stoch_cases as gsc
from tests import gape_stoch_each_cases as ge
from tests import gape_stoch_restatement as gs
from tests.gape_cases import MARGIN, SKIP_CAP
from tests.test_planner_calls_host import GAPE_STOCH_CFG, NO_KIND, UCT, Ctx, Models, plain_env, planner_classes

LDS = 160 * 1024            # bytes of LDS of a compute unit (csrc/common.hpp kLdsBytes): what fits, what the knob can force
DEFAULT = LDS // 16         # kEachLdsDefaultBytes
REC = 16                    # bytes of a packed transition record
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "per_episode_gape_stoch.npz")
MIN_ROOTS = 256             # kGapeLdsMinRoots: the smallest batch at which the LDS form was measured ahead beyond the spread
AB = os.path.join(HERE, "..", "profiles", "gape_stoch_each_ab.json")
BOUND_TOL = 1e-12           # (tests/test_gpu_gape_stoch.py: the same figure, restated here because that module needs a GPU build)
NAMES = ["gape_stoch_each_lds", "gape_stoch_each_lds_slots", "gape_stoch_each_global", "gape_stoch_each_global_slots"]
EXACT = ("parent", "kind", "action", "depth", "count", "done", "cum")
BOUNDS = ("mu_ucb", "mu_lcb", "vu", "vl")


def path_bytes(horizon):
    return 16 * -(-4 * (2 * horizon + 1) // 16)


@pytest.fixture
def no_knob(monkeypatch):
    monkeypatch.delenv("MP_EACH_MODEL", raising=False)


def test_symbols_names_and_abi(no_knob):
    with open(os.path.join(HERE, "..", "include", "mi355plan.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+MP_ABI_VERSION\s+7\b", header)
    lib = native.load()
    assert lib.mp_abi_version() == 7
    for symbol in ("mp_gape_plan_stochastic_models", "mp_gape_stoch_each_form_info"):
        assert symbol in native.SIGNATURES and getattr(lib, symbol) is not None, symbol
        declared = re.search(r"\bint %s\(([^;]*)\);" % symbol, header).group(1)
        assert len(native.SIGNATURES[symbol][1]) == declared.count(",") + 1, symbol
    assert re.search(r"\bconst char \*mp_gape_stoch_each_form_names\(void\);", header)
    assert "mp_gape_stoch_each_form_names" in native.SIGNATURES and lib.mp_gape_stoch_each_form_names is not None
    # model_index in front of the roots, the rest mp_gape_plan_stochastic's in its order
    plain, models = native.SIGNATURES["mp_gape_plan_stochastic"][1], native.SIGNATURES["mp_gape_plan_stochastic_models"][1]
    assert list(models) == list(plain[:3]) + [plain[3]] + list(plain[3:])
    names = native.gape_stoch_each_form_names()
    assert names == NAMES
    others = (native.kernel_form_names(), native.each_form_names(), native.ss_form_names(), native.ss_each_form_names(),
              native.olop_stoch_form_names(), native.gape_form_names(), native.gape_each_form_names(),
              native.gape_stoch_form_names(), native.vi_form_names())
    for other in others:
        assert not set(names) & set(other)
    # the pinned lists are what they were
    assert len(native.kernel_form_names()) == 172 and len(native.each_form_names()) == 8
    assert native.gape_each_form_names() == ["gape_each_lds", "gape_each_lds_slots", "gape_each_global", "gape_each_global_slots"]
    assert len(native.gape_stoch_form_names()) == 6
    assert native.EACH_PLANNERS == {"olop": 0, "brue": 1, "ss": 2}


def test_the_shared_query_does_not_serve_the_new_planner():
    out = np.zeros(6, np.int64)
    for planner in (3, 4):
        assert native.load().mp_each_form_info(planner, 10, 3, 3, 10, 256, out.ctypes.data) == native.MP_ERR_ARG
    for bad in ((0, 3, 3, 10), (10, 0, 3, 10), (10, 3, 0, 10), (10, 3, 3, 0)):
        with pytest.raises(native.NativeError):
            native.gape_stoch_each_form_info(*bad)
    with pytest.raises(native.NativeError):
        native.gape_stoch_each_form_info(10, 3, 3, 10, cus=0)


def test_lds_bytes_default_and_grid(no_knob):
    """The kernel's own arrays are path[2 H + 1] int32, 16-byte rounded; the default is what was measured (each_host.hpp)."""
    assert [path_bytes(h) for h in (1, 2, 3, 4, 6, 8)] == [16, 32, 32, 48, 64, 80]
    for s_each, a, h, n, cus in [(120, 5, 3, 65536, 256), (120, 5, 3, 7, 256), (6, 2, 2, 1000, 256), (1000, 3, 9, 9000, 256),
                                 (2000, 5, 4, 9000, 104), (12, 70, 16, 3, 256), (120, 5, 3, 4096, 256), (1, 1, 1, 1, 1)]:
        info = native.gape_stoch_each_form_info(s_each, a, h, n, cus)
        need = path_bytes(h) + s_each * a * REC
        assert info["lds_bytes"] == need and info["default_limit"] == DEFAULT and info["fit_limit"] == LDS
        lds_per_cu = min(32, LDS // need) if need <= LDS else 0
        # the default (profiles/gape_stoch_each_ab.json): a footprint that leaves 16 wavefronts to a compute unit, from 256 roots
        # on, and only while every root's workgroup is resident at once
        assert info["lds"] == (need <= DEFAULT and MIN_ROOTS <= n <= cus * lds_per_cu)
        assert info["launch_lds_bytes"] == (need if info["lds"] else path_bytes(h))
        assert info["grid"] == min(n, cus * (lds_per_cu if info["lds"] else 32))
    # never the default above kEachLdsDefaultBytes, whatever was measured below it
    assert native.gape_stoch_each_form_info((DEFAULT - 32) // (3 * REC), 3, 3, 1000, 256)["lds"]
    assert not native.gape_stoch_each_form_info((DEFAULT - 32) // (3 * REC) + 1, 3, 3, 1000, 256)["lds"]
    # the highway shape: 17 workgroups of the LDS form to a compute unit
    assert [native.gape_stoch_each_form_info(120, 5, 3, n, 256)["lds"] for n in (1, 255, 256, 4096, 256 * 17, 256 * 17 + 1, 65536)] == \
        [False, False, True, True, True, False, False]
    # the highway shape with the "k2" config: 32 bytes of path + 9.6 KB of records
    assert native.gape_stoch_each_form_info(120, 5, 3, 4096, 256)["lds_bytes"] == 32 + 9600
    # the other MDP-GapE query keeps its own arrays and its own default
    assert native.gape_each_form_info(120, 5, 6, 4096, 256)["lds"] and native.gape_each_form_info(120, 5, 3, 4096, 256)["lds_bytes"] == 16 + 9600


def test_knob_and_fit(monkeypatch):
    monkeypatch.setenv("MP_EACH_MODEL", "lds")
    info = native.gape_stoch_each_form_info(120, 5, 3, 65536, 256)
    assert info["lds"] and info["grid"] == 256 * (LDS // 9632) == 256 * 17 and info["launch_lds_bytes"] == 9632
    assert native.gape_stoch_each_form_info(120, 5, 3, 5, 256)["grid"] == 5
    big = native.gape_stoch_each_form_info(1000, 3, 3, 65536, 256)      # 48 032 bytes: beyond the default limit, forced
    assert big["lds"] and big["lds_bytes"] == 48032 and big["grid"] == 256 * 3
    h = 3
    s_max = (LDS - path_bytes(h)) // (3 * REC)                          # the largest S_each at |A| = 3 that fits, and one more
    fits, over = native.gape_stoch_each_form_info(s_max, 3, h, 1000, 256), native.gape_stoch_each_form_info(s_max + 1, 3, h, 1000, 256)
    assert fits["lds"] and fits["lds_bytes"] <= LDS and fits["grid"] == 256 and fits["launch_lds_bytes"] == fits["lds_bytes"]
    assert not over["lds"] and over["lds_bytes"] > LDS and over["launch_lds_bytes"] == path_bytes(h) and over["grid"] == 1000
    assert native.gape_stoch_each_form_info(1, 3, h, 5, 256)["lds"]
    monkeypatch.setenv("MP_EACH_MODEL", "global")
    info = native.gape_stoch_each_form_info(120, 5, 3, 256, 256)              # (the default at this batch size is the LDS form)
    assert not info["lds"] and info["grid"] == 256 and info["launch_lds_bytes"] == 32 and info["lds_bytes"] == 9632
    monkeypatch.setenv("MP_EACH_MODEL", "something else")
    assert native.gape_stoch_each_form_info(120, 5, 3, 256, 256)["lds"]        # (a value it does not know forces nothing)
    assert not native.gape_stoch_each_form_info(120, 5, 3, 255, 256)["lds"]


def test_the_default_is_what_was_measured(no_knob):
    """profiles/gape_stoch_each_ab.json: the LDS form is the default exactly at the batch sizes where it beat the global form by
    more than the spread between repeated medians; and the plain entry's medians on this tree, set beside the parent commit's
    taken in the same session, are recorded there."""
    import json
    with open(AB) as f:
        doc = json.load(f)
    rows = [r for r in doc if r.get("measure") == "forms"]
    assert [r["roots"] for r in rows] == [1, 256, 4096, 65536] * 2
    for r in rows:
        assert (r["S_each"], r["A"], r["horizon"], r["episodes"], r["accuracy"], r["max_next_states_count"]) == (120, 5, 3, 20, 0.0, 2)
        assert r["bit_identical"]
        g, l = (sum(r[k]) / 2 for k in ("global_ms_medians", "lds_ms_medians"))
        assert r["lds_wins_beyond_spread"] == (g - l > r["spread_ms"])
    # the script was run twice: the LDS form is the default where it won beyond the spread both times
    for roots in (1, 256, 4096, 65536):
        both = [r["lds_wins_beyond_spread"] for r in rows if r["roots"] == roots]
        assert len(both) == 2
        info = native.gape_stoch_each_form_info(120, 5, 3, roots, 256)
        assert info["lds"] == all(both), roots
        assert [r["default_form"] for r in rows if r["roots"] == roots and "default_form" in r] == ["lds" if info["lds"] else "global"]
    plain = [r for r in doc if r.get("measure") == "plain_entry"]
    assert len(plain) == 9 and {r["case"] for r in plain} == {"finite_sparse_b2", "finite_dense8_k8", "finite_det_k2"}
    for r in plain:
        assert len(r["parent_ms_medians"]) == len(r["branch_ms_medians"]) == 6 and r["placement"].startswith("gape_stoch_")


# ---- the planner's call and the opt-in of the per-episode loop -------------------------------------------------------------------
class RecordingCtx(object):
    """Stands where the planner's context is: records which of the two binding methods is called, and with what."""

    def __init__(self):
        self.calls = []

    def gape_plan_stochastic(self, model, roots, episodes, horizon, count, gamma, accuracy, uniform, n_env, column, thr, tthr, vin, rng):
        self.calls.append(("gape_plan_stochastic", None, list(roots), count, n_env, column, len(thr), len(tthr), len(vin)))
        return dict(status=np.zeros(len(roots), np.int32))

    def gape_plan_stochastic_models(self, model, model_index, roots, episodes, horizon, count, gamma, accuracy, uniform, n_env,
                                    column, thr, tthr, vin, rng):
        self.calls.append(("gape_plan_stochastic_models", list(model_index), list(roots), count, n_env, column, len(thr), len(tthr),
                           len(vin)))
        return dict(status=np.zeros(len(roots), np.int32))


def test_plan_on_reaches_the_binding_with_the_model_index():
    from rl_agents_amd.agents.tree_search import mdp_gape
    from rl_agents_amd.gape_stochastic import (PerEpisodeStochasticMDPGapE, PerEpisodeStochasticMDPGapEAgent, StochasticMDPGapE,
                                               StochasticMDPGapEAgent)
    assert PerEpisodeStochasticMDPGapE.__mro__[1] is StochasticMDPGapE
    assert PerEpisodeStochasticMDPGapEAgent.PLANNER_TYPE is PerEpisodeStochasticMDPGapE
    assert issubclass(PerEpisodeStochasticMDPGapEAgent, StochasticMDPGapEAgent)
    # nothing but the three class attributes is the new planner's own: every behaviour is inherited
    own = {k for k in vars(PerEpisodeStochasticMDPGapE) if not k.startswith("__")}
    assert own == {"per_episode_kind", "per_episode_kind_on_request", "plans_on_batch_models"}
    # served by name from the module an agent config names, with no class object among the module's variables
    for name in ("PerEpisodeStochasticMDPGapE", "PerEpisodeStochasticMDPGapEAgent"):
        assert getattr(mdp_gape, name) is {"PerEpisodeStochasticMDPGapE": PerEpisodeStochasticMDPGapE,
                                           "PerEpisodeStochasticMDPGapEAgent": PerEpisodeStochasticMDPGapEAgent}[name]
        assert name not in vars(mdp_gape) and name in dir(mdp_gape)
    model = types.SimpleNamespace(A=3, action_order=np.asarray([2, 0, 1]))
    rng = np.zeros((2, 6), np.uint64)
    cfg = dict(UCT, max_next_states_count=3)
    planner = PerEpisodeStochasticMDPGapE(plain_env(), dict(cfg))
    planner.models = types.SimpleNamespace(ctx=RecordingCtx())
    planner.plan_on(model, [0, 1], [0, 0], rng, model_index=[1, 0], max_plan_len=1)
    planner.plan_on(model, [0, 1], [0, 0], rng)
    with_index, without = planner.models.ctx.calls
    assert with_index[:5] == ("gape_plan_stochastic_models", [1, 0], [0, 1], 3, 3) and with_index[5].tolist() == [1, 2, 0]
    assert with_index[6:] == (UCT["episodes"] + 2, UCT["episodes"] + 2, UCT["horizon"] + 1)
    assert without[0] == "gape_plan_stochastic" and without[2:5] == with_index[2:5] and without[6:] == with_index[6:]
    # the class that was there keeps refusing an index, and makes the same call without one
    old = StochasticMDPGapE(plain_env(), dict(cfg))
    old.models = types.SimpleNamespace(ctx=RecordingCtx())
    with pytest.raises(NotImplementedError, match="one model per episode"):
        old.plan_on(model, [0], [0], rng[:1], model_index=[0])
    old.plan_on(model, [0, 1], [0, 0], rng)
    assert old.models.ctx.calls[0][:5] == without[:5] and old.models.ctx.calls[0][6:] == without[6:]
    # the refusals of the config come first, whatever the index
    for bad, error in ((dict(max_next_states_count=33), NotImplementedError), (dict(max_next_states_count=0), ValueError),
                       (dict(upper_bound=dict(type="hoeffding")), ValueError)):
        refused = PerEpisodeStochasticMDPGapE(plain_env(), dict(cfg, **bad))
        refused.models = types.SimpleNamespace(ctx=RecordingCtx())
        with pytest.raises(error):
            refused.plan_on(model, [0], [0], rng[:1], model_index=[0])
        assert refused.models.ctx.calls == []


def test_without_an_index_the_recorded_call_is_the_one_it_was(monkeypatch):
    """Through the recording stand-in of tests/test_planner_calls_host.py, which binds every call against the real method's
    signature: the new planner class and the old one make the same ``gape_plan_stochastic`` call, argument for argument."""
    from rl_agents_amd.gape_stochastic import PerEpisodeStochasticMDPGapE, StochasticMDPGapE
    monkeypatch.setattr(runtime, "get_context", lambda *a, **k: Ctx.current)
    recorded = []
    for cls in (StochasticMDPGapE, PerEpisodeStochasticMDPGapE):
        planner = cls(plain_env(), dict(GAPE_STOCH_CFG))
        planner.models = Models(Ctx())
        planner.seed(3)
        planner.plan_batch(plain_env(), [0, 1])
        calls = [c for c in planner.models.ctx.calls if c[0].startswith("gape_plan")]
        assert [c[0] for c in calls] == ["gape_plan_stochastic"] and "model_index" not in calls[0][1]
        recorded.append(calls[0][1])
    assert recorded[0] == recorded[1]


def evaluation_of(cls, kind=None, **config):
    env = plain_env()
    config = dict(dict(UCT, max_next_states_count=2), **config)
    planner = cls(env, config)
    planner.models = Models(Ctx())
    return PerEpisodeEvaluation([plain_env(), plain_env()], types.SimpleNamespace(planner=planner, config=config), kind=kind)


def test_kind_on_request(monkeypatch):
    monkeypatch.setattr(runtime, "get_context", lambda *a, **k: Ctx.current)
    from rl_agents_amd.gape_stochastic import PerEpisodeStochasticMDPGapE, StochasticMDPGapE
    classes = planner_classes()
    assert "PerEpisodeStochasticMDPGapE" not in classes and "StochasticMDPGapE" not in classes      # the closed table stays closed
    assert PerEpisodeStochasticMDPGapE.per_episode_kind is None
    assert PerEpisodeStochasticMDPGapE.per_episode_kind_on_request == "gape_stoch"
    assert StochasticMDPGapE.per_episode_kind is None and StochasticMDPGapE.per_episode_kind_on_request is None
    assert classes["MDPGapE"].per_episode_kind is None and classes["MDPGapE"].per_episode_kind_on_request == "gape"
    ev = evaluation_of(PerEpisodeStochasticMDPGapE, kind="gape_stoch")
    assert (ev.kind, ev.subtree, ev.vi) == ("gape_stoch", False, False)
    # unasked: the refusal every planner without a kind gets, to the letter
    with pytest.raises(NotImplementedError) as raised:
        evaluation_of(PerEpisodeStochasticMDPGapE)
    assert str(raised.value) == NO_KIND.format("PerEpisodeStochasticMDPGapE")
    with pytest.raises(NotImplementedError) as raised:
        evaluation_of(StochasticMDPGapE)
    assert str(raised.value) == NO_KIND.format("StochasticMDPGapE")
    with pytest.raises(NotImplementedError, match="step_strategy"):
        evaluation_of(PerEpisodeStochasticMDPGapE, kind="gape_stoch", step_strategy="subtree")
    # a kind another planner declares may not be named, and the old names are offered nothing new
    for cls, kind, offered in ((PerEpisodeStochasticMDPGapE, "gape", "'gape_stoch'"), (StochasticMDPGapE, "gape_stoch", "none"),
                               (StochasticMDPGapE, "gape", "none"), (classes["MDPGapE"], "gape_stoch", "'gape'"),
                               (classes["OLOP"], "gape_stoch", "'olop'")):
        with pytest.raises(ValueError) as raised:
            evaluation_of(cls, kind=kind)
        assert cls.__name__ in str(raised.value) and offered in str(raised.value)
    assert evaluation_of(classes["MDPGapE"], kind="gape", max_next_states_count=1).kind == "gape"


# ---- the fixture of the unmodified reference against the restatement -------------------------------------------------------------
def fixture_case(z, name, e, t):
    n_actions = z["reward"].shape[-1]
    case = dict({"mdp/" + k: z[k][e, t] for k in ("transition", "reward", "terminal")},
                available=np.ones(z["reward"].shape[-2:], bool), order=np.arange(n_actions), done_on_next=False,
                **{k: z["{}/{}".format(name, k)] for k in ("horizon", "episodes", "gamma", "accuracy", "confidence", "continuation",
                                                            "threshold", "transition_threshold", "max_next_states_count")})
    case["mdp/mode"] = np.asarray("deterministic")
    return case


def test_the_fixture_holds_what_it_is_for_and_equals_the_restatement_step_by_step():
    """Margins, an early ending, tie draws and K; then every discrete output of the unmodified reference's per-episode agents, and
    the bounds of the root's arms and of the stored trees within 1e-12 / (1 - gamma): this pins the fixture and the restatement
    to each other without a GPU."""
    z = np.load(GOLDEN)
    assert [str(n) for n in z["configs"]] == ["k2", "k3"]
    for name, horizon, episodes, count in (("k2", 3, 20, 2), ("k3", 4, 30, 3)):
        assert (int(z[name + "/horizon"]), int(z[name + "/episodes"]), float(z[name + "/gamma"]), float(z[name + "/accuracy"]),
                int(z[name + "/max_next_states_count"])) == (horizon, episodes, 0.8, 0.0, count)
        assert str(z[name + "/threshold"]) == "1*np.log(time)" and str(z[name + "/transition_threshold"]) == gsc.DEFAULT_TRANSITION
        assert float(z[name + "/margin"]) > MARGIN
    assert (z["reward"] >= 1e-3).all() and (z["reward"] <= 1 - 1e-3).all()
    n, trees, shortest = len(z["s0"]), 0, {}
    assert n == 7
    for name in ("k2", "k3"):
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
                res, record, seen = gsc.restate_plan(fixture_case(z, name, e, t), int(z["{}/e{}/states".format(name, e)][t]),
                                                     z[p + "/rng_before"])
                assert gsc.margin(seen) > MARGIN, p
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
                    tree = gs.as_bfs(res)
                    for k in EXACT:
                        assert np.array_equal(tree[k], z[p + "/tree/" + k]), (p, k)
                    for k in BOUNDS:
                        assert np.all(np.abs(tree[k] - z[p + "/tree/" + k]) <= BOUND_TOL / (1 - gamma)), (p, k)
                    # placeholders never assigned are in the stored tree: K > 1 on a table
                    assert (z[p + "/tree/action"][z[p + "/tree/kind"] == 0] < -1).any(), p
                    trees += 1
        assert max(lengths) == 3 and min(draws) >= 1, name
        shortest[name] = min(lengths)
    # an episode that ends by its own actions before the last step ("k2" supplies it)
    assert shortest == {"k2": 2, "k3": 3}
    assert trees == 2
    assert os.path.getsize(GOLDEN) < 256 * 1024


# ---- the per-root sweep ----------------------------------------------------------------------------------------------------------
def test_the_sweep_stays_within_its_cap_and_holds_what_it_is_for():
    left_out, plans, counts, rules, continuations, errors = 0, 0, set(), set(), set(), 0
    masked, permuted = [], []
    for i in range(ge.N_CASES):
        case = ge.each_case(i)
        base = case["base"]
        assert str(base["mdp/mode"]) == "deterministic"
        if case["masked"]:          # every table lists other actions: a form that reads another table's flags is caught
            masked.append(i)
            assert len({c["available"].tobytes() for c in case["tables"]}) == ge.TABLES
        else:
            assert all(c["available"].all() for c in case["tables"])
        if not np.array_equal(base["order"], np.arange(len(base["order"]))):
            permuted.append(i)
        assert len({c["mdp/transition"].tobytes() for c in case["tables"]}) == ge.TABLES
        for c in case["tables"]:
            assert (c["mdp/reward"] >= 1e-3).all() and (c["mdp/reward"] <= 1 - 1e-3).all()
            assert int(c["max_next_states_count"]) == int(base["max_next_states_count"])
        counts.add(int(base["max_next_states_count"]))
        rules.add(bool(base["done_on_next"]))
        continuations.add(str(base["continuation"]))
        for res, _, margin in ge.restate_each(case):
            plans += 1
            left_out += not margin > MARGIN
            assert res["error"] in (None, "one_action"), (i, res["error"])        # (a table never runs out of placeholders)
            errors += res["error"] == "one_action"
    assert plans == 95
    print("per-root sweep: {} of {} plans have a margin <= {}".format(left_out, plans, MARGIN))
    assert left_out <= SKIP_CAP * plans
    assert masked == [3, 7, 11, 15] and set(permuted) <= {3, 11} and permuted
    assert counts == {1, 2, 3, 4} and rules == {False, True} and continuations == {"uniform", "zeros"}
    assert errors >= 1
