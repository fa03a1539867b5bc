"""The cases of the MDP-GapE sweep (tests/test_gpu_gape_sweep.py) and the margin rule that decides which of their plans a device
with another ``log`` can be held to -- no GPU needed; tests/test_gape_host.py checks what the sweep contains on the CPU.

``sweep_case(i)``, i < N_RANDOM, is drawn from ``np.random.default_rng(7000 + i)`` over
``generators.random_deterministic(S, A, seed=8000 + i)``; the cases from N_RANDOM on are hand-made for what the drawn ones cannot
hold: the mask sits on i % 3 == 1 and the wide tables on i % 6 == 5, which never meet, and a wide root takes more episodes than
a case has before any node below it is visited twice (HAND_MADE says what each one is for).

A case is a dict in the layout of a golden case (tests/test_gape_host.golden_case), so the helpers made for those read it, plus
``roots`` [ROOTS] and ``rng`` uint64 [ROOTS, 6], a generator record of its own for every root.  Rewards lie in
[1e-3, 1 - 1e-3]: never an exact 0 or 1 (test_goldens_cover_the_issue_cases says why)."""
import numpy as np

from rl_agents_amd import native
from rl_agents_amd.envs import generators
from tests import gape_restatement as gr
from tests.helpers import generator_from

N_RANDOM = 96
ROOTS = 2
MARGIN = 1e-9            # MARGIN of tests/golden/gen/make_golden_gape.py
SKIP_CAP = 0.05          # at most this share of the sweep's plans may have a margin <= MARGIN
HORIZONS, WIDE_HORIZONS = (1, 2, 3, 5, 32, 33, 70), (1, 2, 3)
LOG_TIME = "1*np.log(time)"
NOT_COMPARED = ("continuation", "ties", "arms")     # observations that are no set of compared bounds


def records(rng, n):
    return np.stack([native.rng_state_from_generator(np.random.Generator(np.random.PCG64(int(s))))
                     for s in rng.integers(0, 2 ** 32, size=n)])


def pack(cfg, available, order, done_on_next, roots, rng, **planner):
    a = np.asarray(cfg["reward"]).shape[1]
    return dict({"mdp/" + k: np.asarray(cfg[k]) for k in ("transition", "reward", "terminal")},
                available=np.ones(np.asarray(cfg["reward"]).shape, bool) if available is None else np.asarray(available, bool),
                order=np.arange(a) if order is None else np.asarray(order), done_on_next=bool(done_on_next),
                roots=np.asarray(roots, np.int32), rng=np.asarray(rng, np.uint64), confidence=0.9, max_steps=0, **planner)


def random_case(i):
    rng = np.random.default_rng(7000 + i)
    wide = i % 6 == 5
    n_states = int(rng.integers(2, 40))
    n_actions = int(rng.integers(65, 151)) if wide else int(rng.integers(2, 10))
    cfg = generators.random_deterministic(n_states, n_actions, seed=8000 + i, terminal_rate=float(rng.choice([0.0, 0.2])))
    reward = np.clip(cfg["reward"], 1e-3, 1 - 1e-3)
    if int(rng.integers(3)) == 0:          # a grid of three values: equal cumulative rewards along different paths
        reward = np.clip(np.round(reward * 4) / 4, 0.25, 0.75)
    cfg = dict(cfg, reward=reward)
    available = order = None
    if i % 3 == 1:
        available = generators.random_available(n_states, n_actions, seed=int(rng.integers(2 ** 31)), rate=0.4)
        if i % 2 == 1:
            order = rng.permutation(n_actions)
    horizon = int(rng.choice(WIDE_HORIZONS if wide else HORIZONS))
    episodes = int(rng.integers(1, 6 if horizon >= 32 else 25))
    planner = dict(horizon=horizon, episodes=episodes, gamma=float(rng.choice([0.5, 0.8, 0.9, 0.95])),
                   accuracy=float(rng.choice([0.0, 0.3, 1.0, 2.1])), continuation=str(rng.choice(["uniform", "zeros"])),
                   threshold=str(rng.choice([gr.DEFAULT_THRESHOLD, LOG_TIME])))
    done_on_next = bool(rng.integers(2))
    roots = rng.integers(0, n_states, size=ROOTS)
    return pack(cfg, available, order, done_on_next, roots, records(rng, ROOTS), **planner)


def hand_made(name):
    seed = 9000 + [n for n, _ in HAND_MADE].index(name)
    rng = np.random.default_rng(seed)
    if name in ("wide_masked_uniform", "wide_masked_ordered", "wide_masked_zeros"):
        n_states, n_actions = 9, {"wide_masked_uniform": 150, "wide_masked_ordered": 141, "wide_masked_zeros": 131}[name]
        cfg = generators.random_deterministic(n_states, n_actions, seed=seed)
        cfg = dict(cfg, reward=np.clip(cfg["reward"], 1e-3, 1 - 1e-3))
        available = generators.random_available(n_states, n_actions, seed=seed + 1, rate=0.4)
        order = rng.permutation(n_actions) if name == "wide_masked_ordered" else None
        return pack(cfg, available, order, False, rng.integers(0, n_states, size=ROOTS), records(rng, ROOTS), horizon=3,
                    episodes=12, gamma=0.8, accuracy=0.0, continuation="zeros" if name.endswith("zeros") else "uniform",
                    threshold=LOG_TIME)
    if name in ("wide_below_narrow_root", "wide_below_narrow_root_uniform"):
        # roots that list 2 and 3 actions over states that list 150 and 139: the nodes below the root are visited again and
        # again, and every visit but the first draws among the unvisited children, which all hold the initial value
        n_states, n_actions = 6, 150
        cfg = generators.random_deterministic(n_states, n_actions, seed=seed)
        cfg = dict(cfg, reward=np.clip(cfg["reward"], 1e-3, 1 - 1e-3), transition=2 + cfg["transition"] % (n_states - 2))
        available = np.ones((n_states, n_actions), bool)
        available[0] = available[1] = False
        available[0, [7, 140]] = True
        available[1, [0, 66, 129]] = True
        available[3:, 5:16] = False
        return pack(cfg, available, None, False, [0, 1], records(rng, ROOTS), horizon=3, episodes=20, gamma=0.9, accuracy=0.0,
                    continuation="uniform" if name.endswith("uniform") else "zeros", threshold=LOG_TIME)
    raise KeyError(name)


HAND_MADE = (
    ("wide_masked_uniform", "a mask over 150 actions, uniform continuation: unlisted draws, listed draws in chunks 2 and 3"),
    ("wide_masked_ordered", "the same over 141 actions in a permuted listing order"),
    ("wide_masked_zeros", "a mask over 131 actions, continuation 'zeros': action 0 unlisted at some nodes"),
    ("wide_below_narrow_root", "tie sets of up to 149 members below a root of 2 or 3 arms; the drawn one in every chunk"),
    ("wide_below_narrow_root_uniform", "the same with uniform continuation"),
)
N_CASES = N_RANDOM + len(HAND_MADE)


def sweep_case(i):
    """Case ``i`` of the sweep: the table, availability, listing order, done rule, config, roots and generator records."""
    return random_case(i) if i < N_RANDOM else hand_made(HAND_MADE[i - N_RANDOM][0])


def thresholds(case):
    return gr.thresholds_by_count(str(case["threshold"]), int(case["horizon"]), case["mdp/reward"].shape[1],
                                  float(case["confidence"]), int(case["episodes"]))


def restate_plan(case, s0, rng6, thr=None):
    """The restatement on one root of a case -> (result, generator record after, observations [(kind, values)])."""
    seen = []
    gen = generator_from(rng6)
    res = gr.gape_plan(case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"], int(s0), int(case["episodes"]),
                       int(case["horizon"]), float(case["gamma"]), float(case["accuracy"]), thresholds(case) if thr is None else thr,
                       str(case["continuation"]), gen, available=case["available"], order=case["order"],
                       done_rule="next" if bool(case["done_on_next"]) else "source",
                       observe=lambda kind, values: seen.append((kind, [float(v) for v in values])))
    return res, native.rng_state_from_generator(gen), seen


def restate_case(case):
    thr = thresholds(case)
    return [restate_plan(case, s0, rng6, thr) for s0, rng6 in zip(case["roots"], case["rng"])]


def margin(pairs):
    """The smallest non-zero distance between two finite values of any set the restatement handed to ``observe`` (the "stop"
    pair of bound difference and accuracy is one): the rule of Observers.smallest_margin in
    tests/golden/gen/make_golden_gape.py, on every pair of a set and not only those a scan compares.  Values that are equal are
    equal on the device as well -- the same arithmetic on the same inputs -- and anything further apart than MARGIN compares
    the same way with bounds that are off by 1e-12 / (1 - gamma)."""
    worst = np.inf
    for kind, values in pairs:
        if kind in NOT_COMPARED:
            continue
        v = np.sort(np.asarray([x for x in values if np.isfinite(x)], np.float64))
        d = np.diff(v)
        d = d[d > 0]
        if d.size:
            worst = min(worst, float(d.min()))
    return worst


# ---- the root's best-arm identification in the second and third chunk of 64 lanes ------------------------------------------------
CHUNK_PAIRS = {70: (5, 66), 130: (66, 129), 150: (70, 140)}       # listed root actions -> the two arms with bit-equal bounds


def later_chunk_case(k):
    """``k`` listed root actions, horizon 1, k + 8 episodes: the first-step reward rises with the action, so while unvisited arms
    remain the best arm is the last one visited and the challenger the first unvisited one -- which ties, bit for bit, with every
    later unvisited arm, in its own chunk and in the next.  The two arms of CHUNK_PAIRS[k] share the largest reward: once every
    arm is visited they hold equal bounds in different chunks, the lower one is the best arm and the first largest value_upper,
    the higher one the challenger and the second largest.  (k = 70: arm 67 pays more and is the best arm; the pair ties for
    the challenger and the second largest value_upper, chunk 1 against chunk 2.)"""
    lo, hi = CHUNK_PAIRS[k]
    n_states = 3
    reward = np.tile(0.05 + 0.005 * np.arange(k), (n_states, 1))
    reward[:, [lo, hi]] = 0.9
    if k < 128:
        reward[:, 67] = 0.95      # one chunk past the first: the pair cannot tie across chunks AND hold the best arm in the second
    cfg = dict(transition=(1 + np.arange(k)[None, :] + np.arange(n_states)[:, None]) % n_states, reward=reward,
               terminal=np.zeros(n_states, bool))
    rng = np.random.default_rng(9100 + k)
    return pack(cfg, None, None, False, [0], records(rng, 1), horizon=1, episodes=k + 6, gamma=0.8, accuracy=0.0,
                continuation="zeros", threshold=LOG_TIME)


def tied_positions(values, skipped=None, lowest=False):
    """The positions that hold the largest (or ``lowest``: the smallest) of ``values``, which list the root's arms without
    position ``skipped``."""
    v = np.asarray(values, np.float64)
    at = np.flatnonzero(v == (v.min() if lowest else v.max()))
    return [int(i) + (skipped is not None and i >= skipped) for i in at]


# ---- forged generator words on MDP-GapE's two draws (tests/forge.py) -------------------------------------------------------------
FORGED_KS = (3, 6, 7, 70, 150)
N_FORGED = 28                       # N_TIE of tests/test_gpu_forged_draws.py: every case of forge.TIE_CASES four times
FORGED_STATES = 12
FORGED_PLAN = dict(horizon=2, episodes=4, gamma=0.8, accuracy=0.0, threshold=LOG_TIME)


def forged_table(n_actions, seed):
    cfg = generators.random_deterministic(FORGED_STATES, n_actions, seed=seed)
    return dict(cfg, reward=np.clip(cfg["reward"], 1e-3, 1 - 1e-3))


def forged_continuation_case(k, masked=False):
    """Uniform continuation over ``k`` environment actions: an episode's seed draw takes one word and the first
    ``integers(k)``, at the childless node below the root, the forged ones (forge.tie_batch(k, n, lead=1)).  ``masked``: the
    values the forged words are accepted for, 1 .. 4, are unlisted in every state, with 40 % of the others: rank 0 is taken."""
    from tests import forge
    cfg = forged_table(k, 9200 + k)
    available = None
    if masked:
        available = generators.random_available(FORGED_STATES, k, seed=9300 + k, rate=0.4)
        available[:, 1:5] = False
        available[:, [0, k - 1]] = True
    rng, names = forge.tie_batch(k, N_FORGED, lead=1)
    roots = np.arange(N_FORGED) * 5 % FORGED_STATES
    return pack(cfg, available, None, False, roots, rng, continuation="uniform", **FORGED_PLAN), names


def forged_tie_case(m):
    """Continuation "zeros": the seed draws and the tie draws are the only ones.  States 0 .. 3, the roots, list two actions
    and lead to the others, which list m + 1: the first visit of a node below the root takes its first action, the second one
    draws among the m unvisited children, which all hold the initial value.  Where that draw sits in the stream is read from
    the restatement on forge.LoggingStream; the records put the forged words there.  -> (case, case names, words before)."""
    from tests import forge
    cfg = forged_table(m + 1, 9400 + m)
    cfg["transition"] = 4 + cfg["transition"] % (FORGED_STATES - 4)
    available = np.ones((FORGED_STATES, m + 1), bool)
    available[:4] = False
    available[:4, [0, m]] = True
    roots = np.arange(N_FORGED) % 4
    case = pack(cfg, available, None, False, roots, np.zeros((N_FORGED, 6), np.uint64), continuation="zeros", **FORGED_PLAN)
    words = {first_tie(case, s0, forge.tie_case_record("seeded", m, salt=s0)[0])[0] for s0 in range(4)}
    assert len(words) == 1, words           # no draw before the first tie decides anything: one place for every root and record
    w = words.pop()
    case["rng"], names = forge.tie_batch(m, N_FORGED, skip=w // 2, lead=w % 2)
    return case, names, w


def first_tie(case, s0, rec):
    """(32-bit draws made before, size, rejections) of the first bounded draw of the plan that is not an episode's seed draw."""
    from tests import forge
    stream = forge.LoggingStream(rec)
    gr.gape_plan(case["mdp/transition"], case["mdp/reward"], case["mdp/terminal"], int(s0), int(case["episodes"]),
                 int(case["horizon"]), float(case["gamma"]), float(case["accuracy"]), thresholds(case), str(case["continuation"]),
                 stream, available=case["available"], order=case["order"])
    _, words, _, arg, rejections = [e for e in stream.log if e[3] != 2 ** 30][0]
    return words, arg, rejections
