"""The clone's model-step draw of gape_stoch_kernel ON a cdf entry and one step below it, on dense and sparse rows.

No caller-passed record holds that draw: the planner's record fixes the seed x of the clone the kernel seeds per episode
(seed_sequence.hpp), numpy gives the clone's first double, and the model row it meets is built so that the double sits on
cdf[b] or one step of 2^-53 below it (tests/forge.py, tests/forged_clone_cases.clone_twins, both as they are).  In the first
episode every arm of the root holds the initial bounds, best-arm identification selects the first listed one, and the step of
(root i, action 0) is the forged row.

Held to numpy: the next state the first step observes -- the key of the first placeholder assigned under the root's first arm
-- is ``searchsorted(cdf, u, 'right')`` as ``forge.passed`` / the twin's ``b`` give it; and the whole plan, generator record and
tree against the restatement, whose model steps are numpy's own ``choice(p=row)``."""
import numpy as np
import pytest

from rl_agents_amd import native
from tests import forge
from tests import forged_clone_cases as fc
from tests import gape_restatement as gr
from tests import gape_stoch_cases as gc
from tests import gape_stoch_restatement as gs
from tests.helpers import assert_form
from tests.test_gpu_gape_stoch import assert_tree

pytestmark = pytest.mark.gpu

N_ACTIONS = 3
RUN = dict(episodes=2, horizon=2, gamma=0.8, accuracy=0.0, K=4)


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind,W", [("stochastic", fc.DENSE_W), ("sparse", 3), ("sparse", 4), ("sparse", 5)])
def test_clone_draw_on_and_below_every_threshold(ctx, kind, W):
    batch = fc.clone_twins(kind, W, N_ACTIONS, first="zeros")
    cfg, roots, records = batch["cfg"], batch["roots"], batch["records"]
    cfg = dict(cfg, reward=np.clip(cfg["reward"], 1e-3, 1 - 1e-3))
    model = ctx.load_sparse(cfg["transition"], cfg["next"], cfg["reward"], None) if kind == "sparse" else \
        ctx.load_dense(cfg["transition"], cfg["reward"], None)
    model.set_episode_rules("source", 0)
    episodes, horizon, gamma, K = RUN["episodes"], RUN["horizon"], RUN["gamma"], RUN["K"]
    thr = gr.thresholds_by_count(gc.LOG_TIME, horizon, N_ACTIONS, 0.9, episodes)
    tthr = gs.transition_thresholds_by_count(gc.DEFAULT_TRANSITION, horizon, N_ACTIONS, 0.9, episodes)
    rng = np.ascontiguousarray(records, dtype=np.uint64).copy()
    out = ctx.gape_plan_stochastic(model, roots, episodes, horizon, K, gamma, RUN["accuracy"], False, N_ACTIONS, None, thr, tthr,
                                   gr.value_init(gamma, horizon), rng)
    assert_form(ctx, "gape_stoch_dense" if kind == "stochastic" else "gape_stoch_sparse")
    compared = 0
    for c in batch["cases"]:
        i = c["root"]
        seen = []
        st = forge.Stream(records[i])
        res = gs.gape_stoch_plan(cfg["mode"], cfg["transition"], cfg["reward"], None, int(roots[i]), episodes, horizon, gamma,
                                 RUN["accuracy"], thr, tthr, K, "zeros", st, next_states=cfg["next"],
                                 observe=lambda kind_, values: seen.append((kind_, [float(v) for v in values])))
        # the first step's next state, held to numpy through the forged row: node 1 is the root's first arm (action 0), the K
        # records behind the root's arms are its placeholders, the first of them the first state observed
        assert res["action"][1] == 0 and res["kind"][1 + N_ACTIONS] == 0 and res["parent"][1 + N_ACTIONS] == 1
        observed = int(res["action"][1 + N_ACTIONS])
        if c["b"] is not None:
            want = c["want"] if kind == "stochastic" else int(cfg["next"][c["state"], c["action"], c["want"]])
            assert observed == want, (i, c["b"], c["twin"])
        # the device: generator record and steps always; the rest where no comparison is too close to call
        assert rng[i].tolist() == st.record(), i
        assert int(out["env_steps"][i]) == res["env_steps"], i
        if res["error"]:
            assert res["error"] == "placeholders" and int(out["status"][i]) == native.ERR_GAPE_PLACEHOLDERS, i
            continue
        tree = ctx.gape_stoch_tree(i)
        first_arm = np.flatnonzero((tree["kind"] == 1) & (tree["parent"] == 0))[0]
        kids = np.flatnonzero(tree["parent"] == first_arm)
        assert int(tree["action"][kids[tree["action"][kids] >= 0][0]]) == observed, i     # dict order: placeholders, then observed
        if gc.margin(seen) <= gc.MARGIN:
            continue
        assert int(out["status"][i]) == native.MP_OK and out["plans"][i].tolist() == res["plan"].tolist(), i
        assert int(out["episodes_run"][i]) == res["episodes_run"], i
        assert_tree(tree, gs.as_bfs(res), gamma, i)
        compared += 1
    assert compared >= 0.95 * len(batch["cases"]), (compared, len(batch["cases"]))
    model.close()
