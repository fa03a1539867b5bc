// kl_bound.hpp -- the Kullback-Leibler confidence bound of the empirical mean of rewards in [0, 1] (utils.py:89-203), shared by
// the planners that use it: OLOP's upper bound (olop.hip) and MDP-GapE's two bounds (gape.hip).
#pragma once
#include <math.h>

namespace mp {

// utils.py:89-109 bernoulli_kullback_leibler
__device__ __forceinline__ double bernoulli_kl(double p, double q)
{
    double kl1 = 0.0, kl2 = INFINITY;
    if (p > 0 && q > 0) kl1 = p * log(p / q);
    if (q < 1) kl2 = p < 1 ? (1 - p) * log((1 - p) / (1 - q)) : 0.0;
    return kl1 + kl2;
}

// utils.py:123-146 kl_upper_bound with newton_iteration (:149-203): eps 1e-2, weight 0.9, 100 iterations, the in-loop clamps,
// the final clamp.  `py` follows whether the iterate is still a Python float: only then does the derivative raise
// ZeroDivisionError (and the finite difference of :183 replace it); numpy scalars give inf / nan instead.
// LOWER (utils.py:136-147 with lower=True, MDP-GapE's mu_lcb): count == 0 gives 0, the interval is (a, b) = (0, mu) and the
// start x0 = (0 + mu) / 2.  The kinds of number are those of the upper bound: mu = sum / count is a Python float, so x0 is one
// (`py` starts true); a Newton step subtracts f(x) / df(x), where f(x) went through np.log, and leaves a numpy scalar; a clamp
// weight * a + (1 - weight) * x has the kind of x, for a = 0 (a Python int) as for a = mu.  x0 = mu / 2 is 0 only for mu == 0
// (a == b, returned before the loop) and for the smallest subnormal; there the Python float 0.0 raises in mu / x and the finite
// difference is taken at x - eps < 0, where bernoulli_kl's first term is dropped (q > 0 fails), as on the host.
// TRACE (mp_selftest_olop_bound only; the planners' instantiations are <false> and hold none of it): the number of iterations
// and the decisions taken, KL_* below, so that a test can hold them against the reference's, point by point.
enum { KL_CLAMP_UPPER = 1, KL_CLAMP_LOWER = 2, KL_FINITE_DIFFERENCE = 4, KL_FINAL_LOWER = 8, KL_FINAL_UPPER = 16 };

template <bool TRACE, bool LOWER = false>
__device__ double kl_upper_bound(double total, int count, double threshold, int *iterations = nullptr, int *decisions = nullptr)
{
    int mask = 0, its = 0;
    if constexpr (TRACE) { *iterations = 0; *decisions = 0; }
    if (count == 0) return LOWER ? 0.0 : 1.0;
    const double mu = total / (double)count, max_div = threshold / (double)count;
    const double a = LOWER ? 0.0 : mu, b = LOWER ? mu : 1.0, eps = 1e-2, w = 0.9, wc = 1.0 - 0.9;
    const double x0 = (a + b) / 2;
    if (a == b) return a;
    double x = INFINITY, xn = x0;
    bool pyn = true;
    for (int it = 0; fabs(x - xn) > eps && it < 100; ++it) {
        x = xn;
        const bool px = pyn;
        const double fx = bernoulli_kl(mu, x) - max_div;
        double dfx;
        if (px && (1 - x == 0 || x == 0)) {
            dfx = (fx - (bernoulli_kl(mu, x - eps) - max_div)) / eps;
            if constexpr (TRACE) mask |= KL_FINITE_DIFFERENCE;
        } else dfx = (1 - mu) / (1 - x) - mu / x;
        if (dfx != 0) { xn = x - fx / dfx; pyn = false; }
        if (xn < a) {
            xn = w * a + wc * x; pyn = px;
            if constexpr (TRACE) mask |= KL_CLAMP_LOWER;
        } else if (xn > b) {
            xn = w * b + wc * x; pyn = px;
            if constexpr (TRACE) mask |= KL_CLAMP_UPPER;
        }
        if constexpr (TRACE) ++its;
    }
    if (xn < a) {
        xn = a;
        if constexpr (TRACE) mask |= KL_FINAL_LOWER;
    }
    if (xn > b) {
        xn = b;
        if constexpr (TRACE) mask |= KL_FINAL_UPPER;
    }
    if constexpr (TRACE) { *iterations = its; *decisions = mask; }
    return xn;
}

} // namespace mp
