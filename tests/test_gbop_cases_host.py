"""The cases of tests/gbop_cases.py on the host: every case reaches the edge it is made for IN THE RESTATEMENT -- a case that
stops reaching it fails here instead of passing vacuously on the device -- and the forged ones are tied to numpy.  No GPU needed."""
import numpy as np
import pytest

from tests import forge
from tests import gbop_cases as gc
from tests import gbop_restatement as gb


def call(ref, i, c=0):
    return ref["planners"][i]["calls"][c]


def test_the_diagnostics_count_what_they_say():
    """pushed / peak / update_queue of a call on a graph small enough to follow: every entry pushed is popped, the peak is no
    longer than what was pushed, and the first queue of a run is its update_queue."""
    case, ref = gc.get_case("forms_sparse")
    for p in ref["planners"]:
        c = p["calls"][0]
        assert 1 <= c["uq"] <= c["peak"] <= c["pushed"] <= c["pops"]
        assert c["uq"] <= min(case["calls"][0][2], case["reward"].shape[0])
    graph = gb.Graph("deterministic", np.array([[1], [2], [0]]), np.zeros((3, 1)), 0.8, 1)
    graph.plan(0, 1, 3, 1e-2, lambda c: 0.0, lambda c: 0.0, np.random.default_rng(0))
    assert graph.longest_update_queue == 3 <= graph.pvi_peak and graph.pvi_pushed == graph.pops       # one episode: one queue
    graph.reset_diagnostics()
    assert (graph.longest_update_queue, graph.queue_peak, graph.max_pushed) == (0, 0, 0)


def test_no_case_raises_and_at_most_one_in_ten_is_set_aside():
    for family, (names, _) in gc.FAMILIES.items():
        aside = [n for n in names if gc.set_aside(n)]
        assert len(aside) * 10 <= len(names), (family, aside)
        if family in gc.NEVER_SET_ASIDE:
            assert aside == [], family
        for n in names:
            case, ref = gc.get_case(n)
            assert all(c is not None and c["error"] is None for p in ref["planners"] for c in p["calls"]), n
            assert 3 <= len(ref["planners"]) or family in ("clone", "choice"), n


@pytest.mark.parametrize("name", tuple(gc.WIDE))
def test_wide_cases_try_and_choose_actions_past_the_first_chunk(name):
    case, ref = gc.get_case(name)
    S, A = case["reward"].shape
    assert A > 64
    chosen = []
    for i, p in enumerate(ref["planners"]):
        g, root = p["graph"], int(case["calls"][0][0][i])
        listed = g.listed[root]
        assert all(g.c_count[root, a] > 0 for a in listed), i                 # every root action is tried
        assert sum(gc.slot_of(case, a) >= 64 for a in listed) >= 2, i
        chosen.append(gc.slot_of(case, call(ref, i)["plan"][0]))
    assert max(chosen) >= 64, chosen
    if case["available"] is not None:
        _, _, _, _, av = gc.device_tables(case)
        assert (av[:, :64].sum(axis=1) % 2 == 1).all() and av[:, 63].all() and av[:, 64].all() and av[:, 128:].any(axis=1).all()
        assert not np.array_equal(case["order"], np.arange(A))
        for s in range(S):                                                    # the listing order is the environment's
            assert [gc.slot_of(case, a) for a in ref["planners"][0]["graph"].listed[s]] == np.nonzero(av[s])[0].tolist()


@pytest.mark.parametrize("name", gc.FAMILIES["ring"][0])
def test_ring_cases_queue_more_than_64_states_in_one_episode(name):
    case, ref = gc.get_case(name)
    uq = [call(ref, i)["uq"] for i in range(len(ref["planners"]))]
    assert sum(u > 64 for u in uq) >= 2, uq
    if name.startswith("tail"):
        # the walk comes back to a state it queued past the first 64: the membership scan finds it in its second chunk
        requeue = [call(ref, i)["requeue"] for i in range(len(ref["planners"]))]
        assert sum(r >= 64 for r in requeue) >= 2, requeue
    else:
        assert all(len(p["graph"].created) > 64 for p in ref["planners"])
        assert all(call(ref, i)["requeue"] < 64 for i in range(len(ref["planners"])))           # (what the tail cases add)
    if name == "ring_dense":
        assert case["transition"].shape[2] == gc.RING_S > 64                   # a second ballot in the row search


@pytest.mark.parametrize("name", gc.FAMILIES["hub"][0])
def test_hub_cases_hold_65_parents_and_push_them(name):
    case, ref = gc.get_case(name)
    assert case["calls"][gc.HUB_LAST][1:] == (3, 2) and (case["calls"][gc.HUB_LAST][0] == 0).all()
    for i in (0, 1):
        c = call(ref, i, gc.HUB_LAST)
        assert c["parents_before"][0] >= 65 and c["peak"] >= 65, (i, c["parents_before"][0], c["peak"])
        lst = c["listing"]
        hub = int(np.nonzero(lst["state"] == 0)[0][0])
        assert lst["parent_ptr"][hub + 1] - lst["parent_ptr"][hub] >= 65
    # the two planners met the hub's parents in different orders
    a, b = (call(ref, i, gc.HUB_LAST)["listing"] for i in (0, 1))
    assert a["state"].tolist() != b["state"].tolist()
    small = call(ref, 2, gc.HUB_LAST)
    assert small["parents_before"][0] == 1


@pytest.mark.parametrize("name", gc.FAMILIES["hub"][0])
def test_hub_cases_wrap_the_ring_and_overflow_half_of_it(name):
    case, ref = gc.get_case(name)
    cap, half = gc.queue_caps(ref)
    peaks = [call(ref, i, gc.HUB_LAST)["peak"] for i in range(3)]
    pushed = [call(ref, i, gc.HUB_LAST)["pushed"] for i in range(3)]
    assert cap & (cap - 1) == 0 and cap // 2 < max(peaks) <= cap
    assert max(pushed) > cap                                     # the ring of `cap` entries wraps, and nothing overflows
    assert [p > half for p in peaks] == [True, True, False]      # half of it: two planners overflow, the third fits
    for c in range(gc.HUB_LAST):                                 # the plans before fit both capacities
        assert all(call(ref, i, c)["peak"] <= half for i in range(3)), c
    assert call(ref, 2, gc.HUB_LAST + 1)["peak"] <= half


def test_tail_table_queues_more_states_than_a_ring_of_64_holds():
    case, ref = gc.get_case("tail_table")
    assert [call(ref, i)["uq"] > 64 for i in range(3)] == [True, True, False]
    assert call(ref, 2)["peak"] <= 64


def test_a_full_queue_names_the_settings_this_planner_reads():
    """mp_gbop_create reads MP_GBOP_QUEUE; GBOP-D's message names MP_GBOPD_QUEUE, which this planner never reads."""
    from rl_agents_amd import native
    from rl_agents_amd.gbop import StochasticGraphBasedPlanner
    with pytest.raises(RuntimeError, match="queue overflow") as e:
        StochasticGraphBasedPlanner.raise_for_status(np.asarray([0, native.MP_ERR_ALLOC]))
    assert "StochasticGraphBasedPlanner.queue_capacity" in str(e.value) and "MP_GBOP_QUEUE" in str(e.value)
    assert "MP_GBOPD_QUEUE" not in str(e.value)


def test_limit_cases_stand_on_both_sides_of_the_lds_limit():
    for name, (kind, S) in gc.LIMIT.items():
        case, ref = gc.get_case(name)
        assert case["reward"].shape[0] == S and int(case["calls"][0][0].max()) == S - 1
        assert case["calls"][0][1:] == (6, 5)
    assert {S * 16 <= 16 * 1024 for _, S in gc.LIMIT.values()} == {True, False}


# ---- forged draws
@pytest.mark.parametrize("name", gc.TIE_NAMES)
def test_tie_records_meet_their_rejections(name):
    case, ref = gc.get_case(name)
    k = case["k"]
    assert forge.lemire_threshold(k) > 0                                       # no power of two among the cases
    assert set(case["tie_names"]) == set(forge.TIE_CASES) - {"reject3"}
    met = set()
    for i, p in enumerate(ref["planners"]):
        below = [e for e in p["log"] if e[0] == "below"]
        assert below[0][1:4] == (0, 0, 1 << 30), i                               # the seed word comes first
        assert [e[3] for e in below[1:]] == [k, k, k], i                         # two steps' ties and get_plan's
        want = case["rejections"][i]
        if want is not None:
            assert below[1][4] == want, (i, case["tie_names"][i], below[1])
            met.add(want)
        # numpy's own generator over the same record makes the same plan
        g = gb.Graph(case["mode"], case["transition"], case["reward"], gc.GAMMA, case["K"], None, case["available"])
        gen = gc.generator_from(case["rng"][i])
        plan = g.plan(int(case["calls"][0][0][i]), 1, 2, gc.ACCURACY, lambda c: 0.0,
                      gc.transition_threshold(case["transition_threshold"], 2, case["reward"].shape[1], 1), gen)
        assert plan == call(ref, i)["plan"] and gc.record_of(gen) == call(ref, i)["rng_after"].tolist(), i
    assert met == {0, 1, 2}


@pytest.mark.parametrize("name", tuple(gc.CLONE))
def test_clone_rows_are_met_on_and_below_their_thresholds(name):
    case, ref = gc.get_case(name)
    forged = 0
    for twin, p in zip(case["twins"], ref["planners"]):
        g, i = p["graph"], twin["root"]
        assert int(case["calls"][0][0][i]) == i and p["log"][0][1:4] == (0, 0, 1 << 30), i
        want = gc.clone_want(case, twin)
        if want is None:
            continue
        s, a = twin["state"], twin["action"]
        assert g.c_count[s, a] == 1 and g.c_assigned[s, a] == 1 and g.k_state[s, a, 0] == want, (i, twin["b"], twin["twin"])
        # numpy's search on the row with the clone's own draw; 'left' -- a search written with < for <= -- stops at b for both twins
        u = forge.clone_k53(twin["x"], case["step"]) * 2.0 ** -53
        cdf = np.cumsum(twin["row"])
        assert int(np.searchsorted(cdf / cdf[-1], u, side="right")) == twin["want"]
        assert int(np.searchsorted(cdf / cdf[-1], u, side="left")) == twin["b"]
        forged += 1
    assert forged == (0 if name == "clone_sparse1_0" else len(case["twins"]))
    if case["mode"] == "stochastic":
        assert {t["b"] for t in case["twins"]} >= {0, 63, 64, 127} and case["transition"].shape[2] > 128
    assert {t["x"] for t in case["twins"]} >= {0, 1, (1 << 30) - 1}


@pytest.mark.parametrize("name", gc.CHOICE_NAMES)
def test_choice_records_put_the_draw_on_and_below_the_uniform_cdf(name):
    case, ref = gc.get_case(name)
    K, cdf = case["K"], case["cdf"]
    keys = set()
    for i, (want, p) in enumerate(zip(case["want"], ref["planners"])):
        log = p["log"]
        g, root = p["graph"], int(case["calls"][0][0][i])
        assert [e[0] for e in log] == ["below", "below", "below"] and log[2][2] <= 2 and p["outputs"] == 3, i   # the THIRD output
        assert g.p_minus[root, want["action"]].tolist() == (np.ones(K) / K).tolist(), i
        assert g.c_count[root, want["action"]] == 0, i                                      # an action the episode did not try
        assert call(ref, i)["plan"] == [want["action"], want["key"]], i
        u = want["k53"] * 2.0 ** -53
        if want["b"] is not None:
            c = float(cdf[want["b"]])
            on = want["key"] == "placeholder_{}".format(want["b"] + 1)
            # a cdf entry that is a multiple of 2^-53 is met exactly; the double 1 / 3 is an odd multiple of 2^-54 (2 / 3 is
            # twice that): the draw is the first one above it
            exact = forge.threshold53(c) * 2.0 ** -53 == c
            assert exact == ((K, want["b"]) != (3, 0)), (K, want["b"])
            assert (u == c if exact else u > c) if on else u < c, i
            assert (want["k53"] - 1) * 2.0 ** -53 < c or not on                          # (the draw before it is below)
        keys.add(want["key"])
    assert {"placeholder_0", "placeholder_{}".format(K - 1)} <= keys
    assert ref["choice_margin"] <= 2.0 ** -52 and ref["rest_margin"] > gc.MARGIN


def test_choice_of_a_tried_action_goes_through_the_assigned_slot():
    case, ref = gc.get_case("choice_tried")
    for i, p in enumerate(ref["planners"]):
        g, root = p["graph"], int(case["calls"][0][0][i])
        plan = call(ref, i)["plan"]
        assert g.c_count[root, plan[0]] == 1 and g.c_assigned[root, plan[0]] == 1, i
        assert plan[1] == str(int(g.k_state[root, plan[0], 0])) and g.dict_order(root, plan[0]) == [1, 2, 0], i
    assert ref["choice_margin"] > gc.MARGIN and ref["margin"] > gc.MARGIN
