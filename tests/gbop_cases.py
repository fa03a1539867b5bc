"""The cases of tests/test_gpu_gbop_shapes.py and tests/test_gpu_gbop_forged.py, built on the host and answered by the
restatement (tests/gbop_restatement.py); tests/test_gbop_cases_host.py asserts, without a GPU, that every case reaches the edge
it is made for.  The device tests hand the same cases to mp_gbop_plan and compare as tests/test_gpu_gbop.py's sweep does.

A CASE is a dict: ``mode`` / ``transition`` / ``reward`` / ``next`` (the model in the environment's action ids), ``K``,
``available`` [S, A] and ``order`` (the environment's listing order) or None, ``rng`` (uint64 [n, 6], one record a planner),
``forged`` (the restatement then draws from forge.LoggingStream over the record, else from numpy's Generator), ``calls`` (a list
of (roots [n], episodes, horizon): consecutive plans on ONE kept graph per planner), ``compare`` (the calls after which the
graphs are listed) and ``transition_threshold`` (the config's string).  Everything else is the sweep's: gamma 0.8, accuracy
1e-2, sampling_timeout 100, reward threshold 0.
"""
import functools

import numpy as np

from tests import forge
from tests import forged_clone_cases as fc
from tests import gbop_restatement as gb
from tests.helpers import generator_from, zero_table

GAMMA, ACCURACY, TIMEOUT = 0.8, 1e-2, 100
VMAX = 1 / (1 - GAMMA)
THRESHOLD, TRANSITION_THRESHOLD = "0*np.log(time)", "0.1*np.log(time)"
# ``time`` is the episodes of a plan: with ONE episode the threshold above is 0, and a chance node with one state observed then
# compares log(d) + log(1 / d) -- rounding noise -- with 0 (max_expectation's theta_star).  The one-episode cases take this one.
ONE_EPISODE_THRESHOLD = "0.1*np.log(1 + time)"
MARGIN = 1e-9


class Margin(object):
    """``observe`` of the restatement: the smallest distance of two unequal finite numbers it compared (gb.smallest_margin
    without the list), split into that of get_plan's ``choice`` search and that of everything else."""

    def __init__(self):
        self.choice = self.rest = np.inf

    def __call__(self, kind, a, b):
        a, b = float(a), float(b)
        if a != b and np.isfinite(a) and np.isfinite(b):
            if kind == "choice":
                self.choice = min(self.choice, abs(a - b))
            else:
                self.rest = min(self.rest, abs(a - b))


def transition_threshold(expression, horizon, actions, episodes):
    memo = {}

    def by_count(count):
        if count not in memo:
            memo[count] = gb.thresholds_by_count(expression, horizon, actions, episodes, count, count)[0]
        return memo[count]
    return by_count


def seeded_records(seed, n):
    """The records of numpy's Generator(PCG64(SeedSequence([seed, i]))), i < n."""
    recs = []
    for i in range(n):
        st = np.random.PCG64(np.random.SeedSequence([seed, i])).state
        s, inc = st["state"]["state"], st["state"]["inc"]
        recs.append([s >> 64, s & forge.M64, inc >> 64, inc & forge.M64, st["has_uint32"], st["uinteger"]])
    return np.array(recs, dtype=np.uint64)


def make_case(name, mode, transition, reward, K, rng, calls, next_states=None, available=None, order=None, forged=False,
              compare=None, transition_threshold=TRANSITION_THRESHOLD):
    n = len(rng)
    calls = [(np.asarray(roots, np.int32), int(e), int(h)) for roots, e, h in calls]
    assert all(len(r) == n for r, _, _ in calls)
    return dict(name=name, mode=mode, transition=np.asarray(transition), reward=np.asarray(reward, np.float64), K=int(K),
                next=None if next_states is None else np.asarray(next_states), available=available, order=order,
                rng=np.ascontiguousarray(rng, dtype=np.uint64), forged=forged, calls=calls,
                compare=set([len(calls) - 1] if compare is None else compare), transition_threshold=transition_threshold)


def device_tables(case):
    """What the device is loaded with: the columns in the environment's listing order (column j = action order[j])."""
    t, r, nxt, av, order = case["transition"], case["reward"], case["next"], case["available"], case["order"]
    if order is not None:
        order = np.asarray(order)
        t, r = t[:, order], r[:, order]
        nxt = None if nxt is None else nxt[:, order]
        av = None if av is None else av[:, order]
    return case["mode"], t, r, nxt, av


def restate(case):
    """The restatement's answer -> dict(planners=[dict(graph, calls=[dict(plan, error, rng_after, steps, pops, pushed, peak,
    uq, requeue, parents_before, listing or None)], log and outputs of the forged stream or None)], margin, choice_margin,
    rest_margin).  pushed / peak / uq / requeue are the restatement's diagnostics for that call alone; a planner that raised
    plans no further."""
    A = case["reward"].shape[1]
    watch = Margin()
    planners = []
    for i, rec in enumerate(case["rng"]):
        graph = gb.Graph(case["mode"], case["transition"], case["reward"], GAMMA, case["K"], case["next"], case["available"],
                         case["order"])
        gen = forge.LoggingStream(rec) if case["forged"] else generator_from(rec)
        done, raised = [], None
        for c, (roots, episodes, horizon) in enumerate(case["calls"]):
            if raised is not None:
                done.append(None)
                continue
            graph.reset_diagnostics()
            before = graph.n_observations, graph.pops
            parents_before = [len(p) for p in graph.parents]
            try:
                plan = graph.plan(int(roots[i]), episodes, horizon, ACCURACY, lambda count: 0.0,
                                  transition_threshold(case["transition_threshold"], horizon, A, episodes), gen, TIMEOUT,
                                  observe=watch)
            except ValueError as e:
                plan, raised = [], e
            rng_after = gen.record() if case["forged"] else record_of(gen)
            done.append(dict(plan=plan, error=raised, rng_after=np.array(rng_after, dtype=np.uint64),
                             steps=graph.n_observations - before[0], pops=graph.pops - before[1], pushed=graph.max_pushed,
                             peak=graph.queue_peak, uq=graph.longest_update_queue, requeue=graph.deepest_requeue,
                             parents_before=parents_before,
                             listing=graph.listing() if c in case["compare"] else None))
        planners.append(dict(graph=graph, calls=done, log=gen.log if case["forged"] else None,
                             outputs=gen.outputs if case["forged"] else None))
    return dict(planners=planners, margin=min(watch.rest, watch.choice), choice_margin=watch.choice, rest_margin=watch.rest)


def record_of(gen):
    st = gen.bit_generator.state
    s, inc = st["state"]["state"], st["state"]["inc"]
    return [s >> 64, s & forge.M64, inc >> 64, inc & forge.M64, st["has_uint32"], st["uinteger"]]


# ---- 1. wide and long shapes --------------------------------------------------------------------------------------------------
def random_sparse(seed, S, A, B=2):
    """The sweep's model (tests/test_gpu_gbop.py sweep_model): B successors a row, a self-loop in every state's first action."""
    rng = np.random.default_rng(1000 + seed)
    nxt = rng.integers(0, S, size=(S, A, B))
    nxt[:, 0, 0] = np.arange(S)
    P = rng.dirichlet(np.ones(B), size=(S, A))
    return P, nxt, np.round(rng.random((S, A)), 3)


def dense_of(P, nxt):
    S, A, B = P.shape
    dense = np.zeros((S, A, S))
    for s in range(S):
        for a in range(A):
            for b in range(B):
                dense[s, a, nxt[s, a, b]] += P[s, a, b]
    return dense


WIDE = {"wide70": (40, 5, 70, 2, 80, 3, (0, 2, 4)), "wide150": (41, 7, 150, 3, 160, 2, (1, 3, 6)),
        "wide150_masked": (42, 5, 150, 2, 60, 2, (0, 2, 4))}     # seed, S, A, K, episodes, horizon, roots


def masked_slots(seed, S, A):
    """The slots (positions in the environment's listing) a state lists: an odd number of the first 64, the slots 63 and 64 on
    either side of the chunk border, at least one in the last chunk."""
    rng = np.random.default_rng(seed)
    mask = rng.random((S, A)) < 0.3
    mask[:, 63] = mask[:, 64] = True
    mask[:, A - 1 - np.arange(S) % 3] = True
    for s in range(S):
        if mask[s, :64].sum() % 2 == 0:
            mask[s, s % 60] = not mask[s, s % 60]
    assert (mask[:, :64].sum(axis=1) % 2 == 1).all() and mask[:, 128:].any(axis=1).all()
    return mask


def wide_case(name):
    seed, S, A, K, episodes, horizon, roots = WIDE[name]
    P, nxt, reward = random_sparse(seed, S, A)
    available = order = None
    if name.endswith("_masked"):
        order = np.random.default_rng(seed).permutation(A)
        available = np.zeros((S, A), bool)
        available[:, order] = masked_slots(seed, S, A)          # slot j stands for action order[j]
    return make_case(name, "sparse", P, reward, K, seeded_records(900 + seed, len(roots)), [(roots, episodes, horizon)],
                     next_states=nxt, available=available, order=order)


def slot_of(case, action):
    return int(action) if case["order"] is None else int(np.nonzero(np.asarray(case["order"]) == action)[0][0])


RING_S, RING_ROOTS, TAIL_ROOTS = 80, (0, 27, 79), (6, 15, 24)
TAIL_SPARSE_S, TAIL_SPARSE_ROOTS = 100, (0, 3, 6)
RING_NAMES = ("ring_sparse", "ring_table", "ring_dense", "tail_sparse", "tail_table")


def ring_case(name):
    """ring_*: both actions walk a ring of 80 states one or two steps on, so a walk of 75 steps queues more than 64 distinct
    states.  tail_*: the ring is cut open and its last two states lead to each other, so a walk from the roots above comes
    back to states it queued PAST the first 64 -- the membership scan finds its state in the second chunk."""
    S = TAIL_SPARSE_S if name == "tail_sparse" else RING_S
    s = np.arange(S)
    if name.startswith("tail"):
        one = np.where(s < S - 1, s + 1, S - 2)
        nxt = np.stack([np.stack([one, one[one]], axis=1)] * 2, axis=1)
        P = np.tile(np.array([0.6, 0.4]), (S, 2, 1))
        reward = np.round(np.random.default_rng(51).random((S, 2)), 3)
        calls, rng = [(TAIL_ROOTS, 3, 75)], seeded_records(956, len(TAIL_ROOTS))
        if name == "tail_sparse":                   # (1.4 states a step: a longer chain, from nearer its start)
            return make_case(name, "sparse", P, reward, 2, rng, [(TAIL_SPARSE_ROOTS, 3, 75)], next_states=nxt)
        assert name == "tail_table"
        return make_case(name, "deterministic", nxt[:, :, 0], reward, 1, rng, calls)
    nxt = np.stack([np.stack([(s + 1) % S, (s + 2) % S], axis=1)] * 2, axis=1)        # [S, 2, 2]: both actions walk the ring
    P = np.tile(np.array([0.6, 0.4]), (S, 2, 1))
    reward = np.round(np.random.default_rng(50).random((S, 2)), 3)
    calls, rng = [(RING_ROOTS, 3, 75)], seeded_records(955, len(RING_ROOTS))
    if name == "ring_sparse":
        return make_case(name, "sparse", P, reward, 2, rng, calls, next_states=nxt)
    if name == "ring_dense":
        return make_case(name, "stochastic", dense_of(P, nxt), reward, 2, rng, calls)
    assert name == "ring_table"
    return make_case(name, "deterministic", nxt[:, :, 0], reward, 1, rng, calls)


HUB_S, HUB_P = 72, (0.9, 0.1)
HUB_LAST = 70          # the call that plans the hub itself; one small call follows it


def hub_case(name):
    """Roots 1 .. 70 in turn on one kept graph, 2 episodes of horizon 1 each: state 0 is observed from (nearly) every one of
    them and never expanded, so its parents accumulate while its bounds stay [0, vmax].  Then root 0, 3 episodes of horizon 2:
    its first backup moves its bounds and appends every parent.  Planner 0 takes the roots in ascending order, planner 1 from
    36 on and around, planner 2 plans root 3 every time: its hub has one parent, its queue stays short."""
    S = HUB_S
    s = np.arange(S)
    nxt = np.stack([np.stack([np.zeros(S, np.int64), s], axis=1)] * 2, axis=1)        # [S, 2, 2]: the hub, or stay
    nxt[0, :, 1] = 1
    P = np.tile(np.array(HUB_P), (S, 2, 1))
    reward = np.random.default_rng(60).random((S, 2))     # (not rounded: a self-loop's delta then meets the accuracy exactly)
    calls = [((1 + c, 1 + (c + 35) % 70, 3), 2, 1) for c in range(70)] + [((0, 0, 0), 3, 2), ((0, 5, 3), 2, 1)]
    rng = seeded_records(960, 3)
    compare = (HUB_LAST, HUB_LAST + 1)
    if name == "hub_sparse":
        return make_case(name, "sparse", P, reward, 2, rng, calls, next_states=nxt, compare=compare)
    assert name == "hub_table"
    return make_case(name, "deterministic", nxt[:, :, 0], reward, 1, rng, calls, compare=compare)


def queue_caps(ref):
    """The two capacities of the ring tests from the restatement's numbers for the hub's own plan: the smallest power of two
    that holds every planner's peak, and half of it."""
    peak = max(p["calls"][HUB_LAST]["peak"] for p in ref["planners"])
    cap = 2
    while cap < peak:
        cap *= 2
    return cap, cap // 2


SMALL_FORMS = {"forms_table": ("table", 5, 3, 1), "forms_dense": ("dense", 5, 2, 2), "forms_sparse": ("sparse", 6, 3, 2)}
LIMIT = {"limit_sparse_1024": ("sparse", 1024), "limit_sparse_1025": ("sparse", 1025), "limit_table_1025": ("table", 1025)}


def model_case(name, kind, S, A, K, roots, episodes, horizon, seed):
    P, nxt, reward = random_sparse(seed, S, A)
    calls, rng = [(roots, episodes, horizon)], seeded_records(970 + seed, len(roots))
    if kind == "table":
        return make_case(name, "deterministic", nxt[:, :, 0], reward, K, rng, calls)
    if kind == "dense":
        return make_case(name, "stochastic", dense_of(P, nxt), reward, K, rng, calls)
    return make_case(name, "sparse", P, reward, K, rng, calls, next_states=nxt)


def forms_case(name):
    kind, S, A, K = SMALL_FORMS[name]
    return model_case(name, kind, S, A, K, [i % S for i in (0, 1, 3, S - 1)], 6, 4, 70 + len(kind))


def limit_case(name):
    kind, S = LIMIT[name]
    return model_case(name, kind, S, 2, 2 if kind == "sparse" else 1, (0, S // 3, S // 2 + 1, S - 1), 6, 5, 80 + S % 7)


# ---- 2. forged draws ------------------------------------------------------------------------------------------------------------
# A plan draws, per episode, integers(2 ** 30) (one 32-bit word), per step a tie among the listed actions and the clone's random()
# from its own generator; at the end get_plan's tie and one random() for the weighted choice.
TIE_KS = (3, 6, 7, 70, 150)
TIE_S, TIE_N = 9, 12
TIE_NAMES = tuple("tie_{}_{}".format(kind, k) for kind in ("table", "dense") for k in TIE_KS)


def tie_records(k, n):
    """forge.tie_batch(k, n, lead=1) with the rejections each record prescribes for the first tie (None: the seeded control)."""
    cases = [c for c in forge.TIE_CASES if c != "reject3"]
    expect = []
    for i in range(n):
        inc = (forge.DEFAULT_INC + 2 * i * 0x9E3779B97F4A7C15F39CC0605CEDC834) & forge.M128
        expect.append(forge.tie_case_record(cases[i % len(cases)], k, inc=inc, salt=i // len(cases), lead=1)[1])
    recs, names = forge.tie_batch(k, n, lead=1)
    return recs, names, expect


def tie_case(name):
    """Zero rewards: the sampling rule's and get_plan's decisions are all ties among the k listed actions.  One episode of
    horizon 2: the seed word comes first, the first step's tie meets the forged words, the second starts on whatever half the
    first left."""
    _, kind, k = name.split("_")
    n_actions, k = (8 if int(k) < 8 else int(k)), int(k)
    cfg, (t, r, _), avail = fc.one_hot_tie_model(TIE_S, n_actions, k)
    recs, names, expect = tie_records(k, TIE_N)
    roots = np.arange(TIE_N) % TIE_S
    case = make_case(name, *(("deterministic", t) if kind == "table" else ("stochastic", cfg["transition"])), r, 1, recs,
                     [(roots, 1, 2)], available=avail, forged=True, transition_threshold=ONE_EPISODE_THRESHOLD)
    return dict(case, k=k, tie_names=names, rejections=expect)


CLONE = {"clone_dense_0": ("stochastic", fc.DENSE_W, 0), "clone_dense_1": ("stochastic", fc.DENSE_W, 1),
         "clone_sparse1_0": ("sparse", 1, 0), "clone_sparse3_0": ("sparse", 3, 0), "clone_sparse4_0": ("sparse", 4, 0),
         "clone_sparse5_0": ("sparse", 5, 0), "clone_sparse4_1": ("sparse", 4, 1)}


def clone_case(name):
    """forged_clone_cases.clone_twins as it stands: root i's first tie is among 3 untried actions, below(3) of the record's high
    word; the row that action samples -- or, with ``step`` 1, the row of the second step behind a one-hot row -- sits on, or one
    step below, a threshold of the clone's own draw."""
    kind, W, step = CLONE[name]
    batch = fc.clone_twins(kind, W, 3, first="word", step=step)
    cfg = batch["cfg"]
    case = make_case(name, cfg["mode"], cfg["transition"], cfg["reward"], 2, batch["records"], [(batch["roots"], 1, 1 + step)],
                     next_states=cfg["next"], forged=True, transition_threshold=ONE_EPISODE_THRESHOLD)
    return dict(case, twins=batch["cases"], step=step)


def clone_want(case, twin):
    """The state the forged row's outcome is, or None where the case forges none (a row of one successor)."""
    if twin["b"] is None:
        return None
    return int(twin["want"]) if case["mode"] == "stochastic" else int(case["next"][twin["state"], twin["action"], twin["want"]])


CHOICE_KS = (2, 3, 4, 32)
CHOICE_NAMES = tuple("choice_{}".format(K) for K in CHOICE_KS)
CHOICE_S, CHOICE_A = 6, 3


def choice_record(i, k53, untried, search=64):
    """A record whose THIRD 64-bit output is (k53 << 11 | ..): get_plan's random() on ``zero_table`` after one episode of horizon
    1 -- the seed word and the step's tie are the halves of the first output, get_plan's tie takes a half of the second -- and whose
    get_plan tie picks an action the episode did not try (``untried``) or the one it tried.  The forged state's high word is
    searched for that, as forged_clone_cases.estimate_records does."""
    for j in range(search):
        hi = (fc.hi_of(i) + (j + 1) * 0x2545F4914F6CDD1D) & forge.M64
        rec = forge.double_record(fc.inc_of(i), k53, 0x7ff * (i & 1), hi=hi, skip=2)
        st = forge.Stream(rec)
        st.below(1 << 30)
        first, chosen = st.below(CHOICE_A), st.below(CHOICE_A)
        if st.outputs == 2 and (first != chosen) == untried:
            return rec, chosen
    raise AssertionError("no state found whose get_plan tie picks {} action".format("an untried" if untried else "the tried"))


def choice_case(name):
    """Every lower bound of the root is exactly 0, so get_plan ties among all three actions; where it picks an untried one
    p_minus is uniform 1 / K and every key a placeholder: u on cdf[b] answers placeholder_{b + 1}, one step below placeholder_b."""
    if name == "choice_tried":
        return choice_tried_case()
    K = int(name.split("_")[1])
    t, r, _, _ = zero_table(CHOICE_S, CHOICE_A, CHOICE_A)
    cdf = np.cumsum(np.ones(K) / K)
    cdf /= cdf[-1]
    todo = [(0, 0, None), ((1 << 53) - 1, K - 1, None)]
    for b in sorted({0, K // 2 - 1, K - 2}):
        k53 = forge.threshold53(cdf[b])
        todo += [(k53, b + 1, b), (k53 - 1, b, b)]
    recs, want = [], []
    for i, (k53, placeholder, b) in enumerate(todo):
        rec, action = choice_record(i + 16 * K, k53, True)
        recs.append(rec)
        want.append(dict(k53=k53, action=action, key="placeholder_{}".format(placeholder), b=b))
    case = make_case(name, "deterministic", t, r, K, np.array(recs, dtype=np.uint64), [(np.arange(len(recs)) % CHOICE_S, 1, 1)],
                     forged=True, transition_threshold=ONE_EPISODE_THRESHOLD)
    return dict(case, want=want, cdf=cdf)


def choice_tried_case(name="choice_tried"):
    """The chosen action is the one the episode tried, on a sparse row with K = 3: one child stands for a state (c_m = 1), the
    answer goes through slot (idx + c_m) % K."""
    t, r, _, _ = zero_table(CHOICE_S, CHOICE_A, CHOICE_A)
    nxt = np.stack([t, (t + 2) % CHOICE_S], axis=2)
    P = np.tile(np.array([0.5, 0.5]), (CHOICE_S, CHOICE_A, 1))
    recs = [choice_record(200 + i, (0x15555555555555 + i * 0x3333333333333) & (forge.TWO53 - 1), False)[0] for i in range(4)]
    return make_case(name, "sparse", P, r, 3, np.array(recs, dtype=np.uint64), [(np.arange(4) % CHOICE_S, 1, 1)], next_states=nxt,
                     forged=True, transition_threshold=ONE_EPISODE_THRESHOLD)


FAMILIES = {"wide": (tuple(WIDE), wide_case), "ring": (RING_NAMES, ring_case),
            "hub": (("hub_sparse", "hub_table"), hub_case), "forms": (tuple(SMALL_FORMS), forms_case),
            "limit": (tuple(LIMIT), limit_case), "tie": (TIE_NAMES, tie_case), "clone": (tuple(CLONE), clone_case),
            "choice": (CHOICE_NAMES + ("choice_tried",), choice_case)}
NEVER_SET_ASIDE = ("ring", "hub", "limit")        # (the queue cases are the hub's)
FORM = {"deterministic": "gbop_table", "stochastic": "gbop_dense", "sparse": "gbop_sparse"}


@functools.lru_cache(maxsize=None)
def get_case(name):
    """(case, restatement's answer) by name, computed once a session."""
    for names, build in FAMILIES.values():
        if name in names:
            case = build(name)
            return case, restate(case)
    raise KeyError(name)


def set_aside(name):
    """The margin rule of the sweep: a case in which the restatement compared two unequal numbers closer than MARGIN.  The
    choice cases put get_plan's draw 2^-53 below a cdf entry on purpose -- uniform 1 / K, summed and divided in numpy's order on
    both sides -- so there the rule holds for every other comparison."""
    ref = get_case(name)[1]
    return (ref["rest_margin"] if name in CHOICE_NAMES else ref["margin"]) <= MARGIN
