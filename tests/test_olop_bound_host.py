"""KL-OLOP's bound on the host: the test-side restatement of ``kl_upper_bound`` / ``bernoulli_kullback_leibler`` against the
reference function's own outputs on the lattice of tests/kl_lattice.py (tests/golden/kl_bound.npz), how far one ulp of ``log``
can move the bound, and the plans whose bounds are NaN (tests/golden/olop_nan.npz) -- no GPU needed.

The GPU tests (tests/test_gpu_olop_bound.py) take their premises from here: :func:`sensitivity` (the restatement's iteration
counts and decisions per point, and ``s``) and :func:`log_arguments`.
"""
import functools
import os

import numpy as np
import pytest

from tests import kl_lattice
from tests import olop_restatement as olr
from tests.test_olop_host import golden_case, names, restate, restatement_equals_golden_cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_BOUND = os.path.join(HERE, "golden", "kl_bound.npz")
GOLDEN_NAN = os.path.join(HERE, "golden", "olop_nan.npz")


@functools.lru_cache(maxsize=None)
def lattice():
    lat = kl_lattice.lattice()
    for a in lat.values():
        a.setflags(write=False)
    return lat


def run_lattice(log):
    """The restatement's traced bound on every triple with ``log`` in numpy's place: (bound, iterations, decisions)."""
    lat = lattice()
    out = [olr.kl_upper_bound_traced(float(s), int(c), float(t), log) for s, c, t in zip(lat["total"], lat["count"], lat["threshold"])]
    return (np.asarray([o[0] for o in out], np.float64), np.asarray([o[1] for o in out], np.int32),
            np.asarray([o[2] for o in out], np.int32))


def moved(direction):
    """numpy's log with every finite result replaced by its neighbour towards ``direction`` (log(0) = -inf and NaN are what
    every log returns: they stay)."""
    def log(v):
        with np.errstate(all="ignore"):
            r = np.log(v)
        return np.nextafter(r, direction) if np.isfinite(r) else r
    return log


@functools.lru_cache(maxsize=None)
def sensitivity():
    """dict(base, up, down: (bound, iterations, decisions) of the restatement with numpy's log and with it moved one ulp up /
    down on every call; s: the largest change of a finite bound under either; log_arguments: what the unperturbed run fed to
    log).  Computed once per session."""
    seen = []

    def recording(v):
        seen.append(float(v))
        return np.log(v)

    base = run_lattice(recording)
    up, down = run_lattice(moved(np.inf)), run_lattice(moved(-np.inf))
    fin = np.isfinite(base[0])
    with np.errstate(invalid="ignore"):
        s = max(float(np.abs(up[0] - base[0])[fin].max()), float(np.abs(down[0] - base[0])[fin].max()))
    args = np.unique(np.asarray(seen, np.float64))
    for a in base + up + down + (args,):
        a.setflags(write=False)
    return dict(base=base, up=up, down=down, s=s, log_arguments=args)


def log_arguments():
    return sensitivity()["log_arguments"]


def ulp_error(values, x):
    """|values - log(x)| in ulps of the correctly rounded result, log taken in np.longdouble (64 mantissa bits here, so its own
    error is below 2**-10 ulp of a double); where the true result is inf or NaN: 0 if ``values`` equals it, else inf."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than a double on this host"
    x = np.asarray(x, np.float64)
    values = np.asarray(values, np.float64)
    with np.errstate(all="ignore"):
        true = np.log(x.astype(np.longdouble))
        rounded = true.astype(np.float64)
        fin = np.isfinite(rounded)
        same = (values == rounded) | (np.isnan(values) & np.isnan(rounded))
        err = np.where(same, 0.0, np.inf)
        # one ulp: the spacing of doubles at the true result (np.spacing(0) is the smallest subnormal: log(1) = 0 must be exact)
        err[fin] = (np.abs(values[fin].astype(np.longdouble) - true[fin]) / np.spacing(np.abs(rounded[fin])).astype(np.longdouble))
        err[fin & ~np.isfinite(values)] = np.inf
    return err


def log_ranges():
    """The arguments beside the lattice's own on which a log is measured: (0, 1), just above 1, e**+-700, subnormals and
    1 / (1 - u) -- seeded, 10 000 each."""
    u = np.random.default_rng(21).random((6, 10000))
    return np.concatenate([u[0][u[0] > 0], 1 + 1e-3 * u[1], np.exp(700 * (2 * u[2] - 1)), u[3] * 2.2250738585072014e-308,
                           1 / (1 - u[4]), np.ldexp(0.5 + u[5] / 2, np.arange(10000) % 2098 - 1073),
                           [5e-324, 2.2250738585072014e-308, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0),
                            1.7976931348623157e308, 0.0, -0.0, -1.0, np.inf, -np.inf, np.nan]])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_BOUND)


@pytest.fixture(scope="module")
def znan():
    return np.load(GOLDEN_NAN)


def test_the_lattice_is_the_one_the_golden_was_made_from(golden):
    lat = lattice()
    assert kl_lattice.checksum(lat) == str(golden["checksum"])
    assert len(golden["bound"]) == len(lat["total"]) == len(lat["count"]) == len(lat["threshold"]) >= 30000
    assert len(golden["kl"]) == len(lat["p"]) == len(lat["q"]) >= 3000
    # what the points are there for: NaN bounds, the NaN threshold, q >= 1, p and q at and one ulp from 0 and 1
    assert np.isnan(golden["bound"]).sum() >= 1900 and np.isnan(lat["threshold"]).any()
    assert (lat["q"] >= 1).any() and np.isinf(golden["kl"]).any() and np.isnan(golden["kl"]).any() and (golden["kl"] == 0).any()
    for edge in (0.0, 5e-324, 1.0, np.nextafter(1.0, 0.0)):
        assert (lat["p"] == edge).any() and (lat["q"] == edge).any()
    assert golden["bound"].nbytes + golden["kl"].nbytes < 300 * 1024


def test_restated_bound_equals_the_reference_function(golden):
    bound = sensitivity()["base"][0]
    assert np.array_equal(np.isnan(bound), np.isnan(golden["bound"]))
    assert np.array_equal(bound.view(np.uint64)[~np.isnan(bound)], golden["bound"].view(np.uint64)[~np.isnan(bound)])
    lat = lattice()
    # a NaN threshold gives a NaN bound wherever the Newton iteration runs at all
    runs = np.isnan(lat["threshold"]) & (lat["total"] != lat["count"])
    assert runs.sum() > 1000 and np.isnan(golden["bound"][runs]).all()


def test_restated_divergence_equals_the_reference_function(golden):
    lat = lattice()
    with np.errstate(all="ignore"):
        kl = np.asarray([olr._bernoulli_kl(float(p), float(q)) for p, q in zip(lat["p"], lat["q"])], np.float64)
    assert np.array_equal(np.isnan(kl), np.isnan(golden["kl"]))
    assert np.array_equal(kl.view(np.uint64)[~np.isnan(kl)], golden["kl"].view(np.uint64)[~np.isnan(kl)])


def test_one_ulp_of_log_changes_no_decision():
    """The premise of holding a device with its own log to 1e-12: with every log result moved to its upper neighbour, or to
    its lower one, the Newton iteration stops after the same number of steps and takes the same clamps and the same finite
    differences on EVERY point of the lattice (none is excluded), so the bound moves by rounding only."""
    sens = sensitivity()
    bound, its, mask = sens["base"]
    for other in ("up", "down"):
        b2, its2, mask2 = sens[other]
        assert np.array_equal(its, its2), (other, np.flatnonzero(its != its2)[:5])
        assert np.array_equal(mask, mask2), (other, np.flatnonzero(mask != mask2)[:5])
        assert np.array_equal(np.isnan(bound), np.isnan(b2)) and np.array_equal(np.isinf(bound), np.isinf(b2)), other
    print("s = max |change of a finite bound| = {:.3e}".format(sens["s"]))
    assert 0 < sens["s"] <= 2.5e-13          # (4 s is the GPU test's tolerance: it has to say something below 1e-12)
    # the lattice reaches what it is for
    assert its.min() == 0 and its.max() >= 5 and len(np.unique(its)) >= 6     # lanes of a wave run different counts
    assert (mask & olr.KL_CLAMP_UPPER).astype(bool).sum() > 5000
    nan = np.isnan(bound)
    fd = (mask & olr.KL_FINITE_DIFFERENCE).astype(bool)
    lat = lattice()
    assert fd.sum() > 500 and np.isnan(bound[fd & ~np.isnan(lat["threshold"])]).all()
    assert nan[~np.isnan(lat["threshold"])].sum() == (fd & ~np.isnan(lat["threshold"])).sum()


def test_numpy_log_is_within_one_ulp_of_a_long_double_log():
    for x in (log_arguments(), log_ranges()):
        with np.errstate(all="ignore"):
            err = ulp_error(np.log(x), x)
        print("numpy log: {} arguments, max error {:.4f} ulp".format(len(x), err.max()))
        assert err.max() <= 1.0


def test_restated_plans_with_nan_bounds_equal_the_reference(znan):
    assert restatement_equals_golden_cases(znan) == len(names(znan)) == 10


def test_every_nan_case_reaches_the_nan_paths(znan):
    """A later change of tables must not lose the path silently: each case has NaN mu_ucb, a NaN first child beside a finite
    sibling (the first-element rule of Python's max, olop.py:84), and a parent whose value_upper is NaN because ONE of its
    children's is (np.amax, olop.py:188) while a sibling's is finite."""
    conts = set()
    for name in names(znan):
        case = golden_case(znan, name)
        conts.add(str(case["continuation"]))
        mu, vu, parent = case["tree/mu"], case["tree/vu"], case["tree/parent"]
        assert np.isnan(mu).sum() >= 3, name
        kids = {}
        for i, p in enumerate(parent):
            if p >= 0:
                kids.setdefault(int(p), []).append(i)
        first_nan = [p for p, k in kids.items() if np.isnan(vu[k[0]]) and np.isfinite(vu[k[1:]]).any()]
        mixed = [p for p, k in kids.items() if np.isnan(vu[k]).any() and np.isfinite(vu[k]).any() and np.isnan(vu[p])]
        assert mixed, name
        if name.startswith(("first", "every", "ordered")):
            assert first_nan, name
    assert conts == {"uniform", "zeros"}
    every = golden_case(znan, "every_uniform")
    assert every["mdp/reward"].shape[1] == 5 and (every["mdp/reward"] == kl_lattice.ULP_BELOW_ONE).all()
    ordered = golden_case(znan, "ordered_zeros")
    assert not ordered["available"].all() and not np.array_equal(ordered["order"], np.arange(5))


def test_the_nan_cases_tell_a_wrong_nan_rule_from_the_right_one(znan):
    """What olop.hip would compute without its two NaN lines, restated: a selection that skips a NaN first child (the
    strict-max loop of olop_first_max without its ``isnan(V[first])`` return) and a backup maximum that ignores NaN children
    (olop_amax without its ``nan_seen`` ballot; -inf when all are NaN).  Each must change the tree of some golden case -- so the
    plan-level GPU tests, which expect the goldens' trees, would fail on such a kernel."""
    def skipping_first_max(values):
        best, idx = None, len(values)          # (all NaN: no lane has a value and the kernel's index is out of range)
        for i, v in enumerate(values):
            if not np.isnan(v) and (best is None or v > best):
                best, idx = v, i
        return idx if best is not None else 0

    def nan_blind_amax(values):
        v = np.asarray(values, np.float64)
        return v[~np.isnan(v)].max() if (~np.isnan(v)).any() else -np.inf

    told = {"first_max": [], "amax": []}
    for name in names(znan):
        case = golden_case(znan, name)
        for rule, kwargs in (("first_max", dict(first_max=skipping_first_max)), ("amax", dict(amax=nan_blind_amax))):
            res, _ = restate(case, **kwargs)
            tree = olr.as_bfs(res)
            same = all(np.array_equal(tree[k], case["tree/" + k], equal_nan=True) for k in ("parent", "action", "count", "cum", "mu", "vu"))
            if not same:
                told[rule].append(name)
    assert told["first_max"] == told["amax"] == names(znan), told
