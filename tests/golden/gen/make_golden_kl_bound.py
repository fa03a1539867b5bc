#!/usr/bin/env python3
"""Golden vectors for KL-OLOP's bound: the UNMODIFIED reference ``rl_agents.utils.kl_upper_bound`` (with its
``newton_iteration``) on every triple of ``tests/kl_lattice.py`` and ``bernoulli_kullback_leibler`` on its pairs.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_kl_bound.py      (build container only)

-> tests/golden/kl_bound.npz: ``bound`` [n] and ``kl`` [m] float64, what the reference returned (NaN where it returned NaN),
and ``checksum``, the sha256 of the inputs they belong to.  Nothing of the reference is copied: its outputs only; the inputs
are rebuilt by ``kl_lattice.lattice()`` wherever they are needed.

``np.infty`` (removed in numpy 2, utils.py:97) is aliased to ``np.inf`` before the reference is imported, and the reference is
imported through the stub packages of ``make_golden.py``; neither changes what it computes.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (puts the stubs, the reference and this repository on sys.path)
from make_golden import np  # noqa: E402

np.infty = np.inf
from rl_agents import utils as ref_utils  # noqa: E402

from tests import kl_lattice  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "kl_bound.npz"))


def main():
    lat = kl_lattice.lattice()
    warnings.simplefilter("ignore")          # divisions by zero and inf - inf are what the edge points are for
    with np.errstate(all="ignore"):
        bound = np.asarray([float(ref_utils.kl_upper_bound(float(s), int(c), float(t)))
                            for s, c, t in zip(lat["total"], lat["count"], lat["threshold"])], np.float64)
        kl = np.asarray([float(ref_utils.bernoulli_kullback_leibler(float(p), float(q))) for p, q in zip(lat["p"], lat["q"])],
                        np.float64)
    np.savez_compressed(OUT, bound=bound, kl=kl, checksum=np.asarray(kl_lattice.checksum(lat)))
    print("wrote", OUT, len(bound), "bounds,", int(np.isnan(bound).sum()), "NaN;", len(kl), "divergences,",
          int(np.isinf(kl).sum()), "inf,", int(np.isnan(kl).sum()), "NaN;", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
