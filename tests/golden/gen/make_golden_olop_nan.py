#!/usr/bin/env python3
"""Golden vectors for the NaN bounds of KL-OLOP: the UNMODIFIED reference ``OLOPAgent`` (through ``make_golden_olop.one_plan``
and its adapters) on tables whose rewards make ``kl_upper_bound`` return NaN.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen/make_golden_olop_nan.py      (build container only)

A reward of 1 - 2**-53 puts mu = cumulative_reward / count one ulp below 1; the Newton iteration's first iterate
(mu + 1) / 2 rounds to exactly 1.0, the derivative raises ZeroDivisionError (utils.py:188) and the finite difference that
replaces it is inf / inf.  The NaN mu_ucb then meets Python's ``max`` in the selection (olop.py:84, a NaN first child stays),
``np.amax`` in the backup (olop.py:188, NaN propagates) and ``selection_rule`` in the plan.

-> tests/golden/olop_nan.npz, in the layout of olop.npz: per case the MDP, the config, the generator records, the plan, the whole
tree and ``get_visits()``.  Inputs and the reference's outputs only.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_olop as mgo  # noqa: E402
from make_golden_olop import generators, np  # noqa: E402

OUT = os.path.abspath(os.path.join(HERE, "..", "olop_nan.npz"))
NAN_MAKING = 1.0 - 2.0 ** -53


def table(states, actions, seed, columns):
    tab = generators.random_deterministic(states, actions, seed=seed, terminal_rate=0.1)
    reward = np.asarray(tab["reward"], np.float64).copy()
    reward[:, columns] = NAN_MAKING
    return dict(tab, reward=reward)


def main():
    store, names = {}, []
    kl = {"type": "kullback-leibler"}
    avail = generators.random_available(12, 5, seed=9, rate=0.3)
    avail[:, 0] = True                      # the "zeros" continuation needs action 0 among the children
    cases = [
        # name, table, episodes, available, listing order.  (A NaN first child is chosen again and again, olop.py:84, and
        # the sum of k such rewards over k is NaN-making for k = 1-4, 6-8, 11-16 but not for 5, 9, 10: hence 8 episodes.)
        ("first", table(12, 3, 1, [0]), 8, None, None),
        ("middle", table(12, 3, 2, [1]), 9, None, None),
        ("last", table(12, 3, 3, [2]), 9, None, None),
        ("every", table(12, 5, 4, slice(None)), 9, None, None),
        ("ordered", table(12, 5, 5, [0, 3]), 9, avail, [3, 1, 0, 4, 2]),  # a NaN-making action listed first, another third
    ]
    seed = 30
    for name, tab, episodes, available, order in cases:
        for cont in ("uniform", "zeros"):
            cfg = dict(horizon=4, episodes=episodes, gamma=0.8, continuation_type=cont, upper_bound=kl)
            mgo.one_plan(store, "olop/{}_{}".format(name, cont), tab, 0, cfg, seed, available, order, 0)
            names.append("{}_{}".format(name, cont))
            seed += 1
    store["olop/names"] = np.asarray(names)
    np.savez_compressed(OUT, **store)
    for n in names:
        print(n, "error", repr(str(store["olop/" + n + "/error"])), "nodes", len(store["olop/" + n + "/tree/mu"]), "NaN mu",
              int(np.isnan(store["olop/" + n + "/tree/mu"]).sum()), "NaN value_upper", int(np.isnan(store["olop/" + n + "/tree/vu"]).sum()),
              "plan", store["olop/" + n + "/plan"].tolist())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
