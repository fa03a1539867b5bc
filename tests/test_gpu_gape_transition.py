"""The device's transition bound (rl_agents_amd/csrc/kl_transition.hpp through mp_selftest_gape_transition) against the
reference's ``max_expectation_under_constraint`` on the lattice of tests/golden/gape_transition.npz.

At every point that does not carry the file's flag (the reference's own result moves by more than 1e-13 under a 2-ulp jitter
of log / exp; at most 5 % of the lattice): the branches taken and the Newton iteration count are the reference's, and p_star is
within 1e-12, the project's number for the KL bound (the largest deviation seen is recorded there).

What the cap hides: the lattice holds few points at ``c == 0`` (one per kind of ``f`` and width, 25 of 664, 10 of them flagged), because the
reference is unstable at most of them -- theta's root is at infinity -- and they carry the flag.  The cap of 5 % is met by that
choice of lattice, not by the device, and the device is checked at ``c == 0`` only at the handful of such points that are
stable (the ``isclose`` and zero-mass branches, which take no Newton step)."""
import numpy as np
import pytest

from rl_agents_amd import native
from tests.test_gape_stoch_host import TRANSITION

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 5, 32, "_hand")       # the lattice by width, and the hand-made points of width 4 (the beta == 0 branches)
P_TOL = 1e-12
FLAG_CAP = 0.05


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lattice():
    return np.load(TRANSITION)


def test_flagged_share_is_within_the_cap(lattice):
    n = sum(len(lattice["c%s" % K]) for K in WIDTHS)
    flagged = sum(int(lattice["flag%s" % K].sum()) for K in WIDTHS)
    assert flagged <= FLAG_CAP * n, (flagged, n)


@pytest.mark.parametrize("K", WIDTHS)
def test_device_transition_bound_on_the_lattice(ctx, lattice, K):
    f, q, c = lattice["f%s" % K], lattice["q%s" % K], lattice["c%s" % K]
    p, its, mask = ctx.selftest_gape_transition(f, q, c)
    keep = ~lattice["flag%s" % K]
    want = lattice["p%s" % K]
    assert np.array_equal(np.isnan(p[keep]), np.isnan(want[keep])), K
    err = np.nanmax(np.abs(p[keep] - want[keep]), initial=0.0)
    wrong = np.flatnonzero(keep & ((its != lattice["iterations%s" % K]) | (mask != lattice["decisions%s" % K])))
    print("K {}: {} of {} points checked, max |device - reference| = {:.3g}, trace differs at {}".format(
        K, int(keep.sum()), len(c), err, wrong.tolist()))
    assert wrong.size == 0, (K, wrong.tolist(), its[wrong].tolist(), lattice["iterations%s" % K][wrong].tolist(),
                             mask[wrong].tolist(), lattice["decisions%s" % K][wrong].tolist())
    assert err <= P_TOL, (K, err)
    # a distribution wherever the reference's is one
    sums = want[keep].sum(axis=1)
    ok = np.isfinite(sums)
    assert np.all(np.abs(p[keep].sum(axis=1)[ok] - sums[ok]) <= f.shape[1] * P_TOL), K


def test_an_odd_number_of_problems_and_refusals(ctx, lattice):
    """Two problems share a wavefront: the last of an odd number sits alone in its wavefront, beside an idle half."""
    f, q, c = lattice["f5"][:7], lattice["q5"][:7], lattice["c5"][:7]
    p7, its7, mask7 = ctx.selftest_gape_transition(f, q, c)
    for i in range(7):
        p1, its1, mask1 = ctx.selftest_gape_transition(f[i:i + 1], q[i:i + 1], c[i:i + 1])
        assert np.array_equal(p1[0], p7[i], equal_nan=True) and its1[0] == its7[i] and mask1[0] == mask7[i], i
    with pytest.raises(native.NativeError, match="width"):
        ctx.selftest_gape_transition(np.zeros((1, 33)), np.zeros((1, 33)), np.zeros(1))
