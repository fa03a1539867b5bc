// kl_transition.hpp -- the transition bound of MDP-GapE's chance nodes: max over p of E_p[f] subject to KL(q || p) <= c
// (utils.py:292-342 max_expectation_under_constraint, with theta_func / d_theta_dl_func :279-289 and the newton_iteration call of
// :330: x0 = f_star + 1, a = f_star, no b, eps 1e-2, weight 0.9, 100 iterations), for at most 32 entries.
//
// Mapping: ONE PROBLEM PER HALF of a wavefront.  Lane l holds entry (l & 31) of the problem of half (l >> 5); every reduction
// (q_p @ log(l - f_p), q_p @ (1 / (l - f_p)), q_p @ (1 / (l - f_p))**2, the maxima, the counts) runs over the 32 lanes of a half:
// butterfly shuffles of distance <= 16 and ballots masked to the half.  A chance node's upper solve (f = u_next) and lower solve
// (f = -l_next) are independent, so gape_stoch_kernel runs them side by side in the two halves; the Newton loop goes on while
// EITHER half has not stopped, each half predicated on its own test.  Control flow is uniform within a half everywhere.
//
// numpy semantics, branch by branch: a division by zero is inf, an invalid operation NaN, nothing raises; `df_x != 0` is true
// for NaN; np.amax is NaN where an entry is; np.isclose(a, b) is |a - b| <= 1e-8 + 1e-5 * |b| for finite numbers and a == b else.
// The sums take the butterfly's order, not numpy's pairwise / BLAS order, and log / exp are the device's: p_star agrees with the
// reference to rounding, not bit for bit.
// TRACE (mp_selftest_gape_transition only; the planner's instantiation is <false>): the Newton iterations and the KT_* decisions.
#pragma once
#include <math.h>

namespace mp {

enum {
    KT_UNIFORM_Q = 1,      // q was all zeros and became uniform (:305-306)
    KT_FSTAR_ABOVE = 2,    // f_star > amax(f_p): the largest f sits on a zero-probability entry (:317)
    KT_ZERO_MASS = 4,      // ... and theta_star < 0: mass z on the zero-probability maxima, lambda = f_star (:319-323)
    KT_ISCLOSE = 8,        // every f_p isclose to the first: q is returned (:325-326)
    KT_NEWTON = 16,        // lambda from the Newton iteration (:330)
    KT_CLAMP = 32,         // an iterate fell below a and was pulled back (:193-194)
    KT_FINAL_CLAMP = 64,   // the last iterate was below a (:198-199)
    KT_BETA_ZERO = 128,    // beta == 0 (:336)
    KT_BETA_UNIFORM = 256  // ... and the mass went to the positive-probability maxima (:337-339)
};

__device__ __forceinline__ double kt_half_sum(double v)
{
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// np.amax over the lanes of a half where `in`: NaN if any is NaN, -inf over none
__device__ __forceinline__ double kt_half_amax(bool in, double v, unsigned long long half_mask)
{
    double m = in && !isnan(v) ? v : -INFINITY;
    for (int off = 16; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    return (__ballot(in && isnan(v)) & half_mask) ? (double)NAN : m;
}

__device__ __forceinline__ bool kt_isclose(double a, double b)
{
    if (isfinite(a) && isfinite(b)) return fabs(a - b) <= 1e-8 + 1e-5 * fabs(b);
    return a == b;
}

// p_star of this lane's entry (0 for an entry >= K).  Every lane of the wavefront calls it; f, q are the lane's, c and K the
// half's (1 <= K <= 32).  *iterations / *decisions (TRACE): the half's, the same in each of its lanes.
template <bool TRACE>
__device__ double kl_transition_p(double f, double q, double c, int K, int lane, int *iterations = nullptr, int *decisions = nullptr)
{
    const unsigned long long half_mask = lane < 32 ? 0xffffffffull : 0xffffffff00000000ull;
    const int li = lane & 31, base = lane & 32;
    const bool in = li < K;
    const double eps = 1e-2, w = 0.9, wc = 1.0 - 0.9;
    int mask = 0, its = 0;
    auto count = [&](bool pred) { return __popcll(__ballot(pred) & half_mask); };

    if (count(in && q == 0) == K) { // np.all(q == 0)
        q = 1.0 / (double)K;
        mask |= KT_UNIFORM_Q;
    }
    const bool plus = in && q > 0, zero = in && q == 0;
    const double f_star = kt_half_amax(in, f, half_mask), fp_max = kt_half_amax(plus, f, half_mask);
    // theta (:279-282) and the two sums of its derivative (:285-289) at x
    auto sums = [&](double x, double *s1, double *s2) {
        const double d = x - f, inv = 1.0 / d;
        const double s_log = kt_half_sum(plus ? q * log(d) : 0.0);
        *s1 = kt_half_sum(plus ? q * inv : 0.0);
        *s2 = kt_half_sum(plus ? q * (inv * inv) : 0.0);
        return s_log + log(*s1) - c;
    };
    double p = 0.0, lam = 0.0, z = 0.0;
    bool have_lambda = false;
    if (f_star > fp_max) {
        mask |= KT_FSTAR_ABOVE;
        double s1, s2;
        const double theta_star = sums(f_star, &s1, &s2);
        if (theta_star < 0) {
            mask |= KT_ZERO_MASS;
            have_lambda = true;
            lam = f_star;
            z = 1.0 - exp(theta_star);
            // f_star > amax(f_p) sits among the zero-probability entries: amax(f[x_zero]) is f_star
            const bool top = zero && f == f_star;
            const double share = z / (double)count(top);
            if (top) p = 1.0 * share;
        }
    }
    bool newton = false;
    if (!have_lambda) {
        const unsigned long long pl = __ballot(plus) & half_mask;
        const double f0 = __shfl(f, pl ? __ffsll((long long)pl) - 1 : base); // f_p[0]
        if (count(plus && !kt_isclose(f, f0)) == 0) {
            if constexpr (TRACE) { *iterations = 0; *decisions = mask | KT_ISCLOSE; }
            return in ? q : 0.0;
        }
        newton = true;
        mask |= KT_NEWTON;
    }
    // newton_iteration (:150-203): one loop for both halves
    const double a = f_star;
    double x = INFINITY, xn = f_star + 1.0;
    for (;;) {
        const bool go = newton && fabs(x - xn) > eps && its < 100;
        if (!__any(go)) break;
        double s1, s2;
        const double fx = sums(xn, &s1, &s2);
        if (go) {
            ++its;
            x = xn;
            const double dfx = s1 - s2 / s1;
            if (dfx != 0) xn = x - fx / dfx;
            if (xn < a) {
                xn = w * a + wc * x;
                mask |= KT_CLAMP;
            }
        }
    }
    if (newton) {
        if (xn < a) {
            xn = a;
            mask |= KT_FINAL_CLAMP;
        }
        lam = xn;
    }
    const double beta = (1.0 - z) / kt_half_sum(plus ? q * (1.0 / (lam - f)) : 0.0);
    if (beta == 0) {
        mask |= KT_BETA_ZERO;
        const bool uni = in && q > 0 && f == f_star;
        const int n_uni = count(uni);
        if (n_uni > 0) {
            mask |= KT_BETA_UNIFORM;
            if (uni) p = (1.0 - z) / (double)n_uni;
        }
    } else if (plus) p = beta * q / (lam - f);
    if constexpr (TRACE) { *iterations = its; *decisions = mask; }
    return p;
}

} // namespace mp
