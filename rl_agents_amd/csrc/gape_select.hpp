// gape_select.hpp -- what the two MDP-GapE kernels (gape.hip, gape_stoch.hip) do alike over a decision node's chance children,
// whose values lie as C = [k][2] (value_upper, value_lower), 64 lanes at a time: the first maximum, best-arm identification at
// the root (mdp_gape.py:228-249), np.amax of a column (:219-220) and random_argmax over value_upper (:189-192).  Everything else
// the two share, host side included, is in gape_shared.hpp, which includes this header.
#pragma once
#include <math.h>

#include "pcg64.hpp"

namespace mp {

// the first maximum of f(i) over [0, k), NaN never winning (`v > best` is false for it); f gives -inf where i is left out.
// The index is ALWAYS in [0, k): where nothing exceeds -inf -- every value left out, -inf or NaN -- it is `fallback`, which the
// caller chooses among the indices it has not left out.
template <typename F>
__device__ __forceinline__ int gape_first_max(int k, int lane, int fallback, F f, double *value = nullptr)
{
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < k; i += 64) {
        const double v = f(i);
        if (v > bv) { bv = v; bi = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (value) *value = bv;
    return bi < k ? bi : fallback;
}

// best_arm_identification_selection (mdp_gape.py:228-249) over k >= 2 children, C = [k][2] (value_upper, value_lower).
// gap_i = max over j != i of (U_j - L_i), from -inf with Python's max(a, b), which a NaN term never replaces: rounding is
// monotone, so that is (max over the non-NaN U_j, j != i) - L_i, -inf where that difference is NaN; and the maximum without i
// is the largest U, or the second largest where i is the first to hold the largest.  min() by gap keeps the first minimum (no
// gap is NaN); max() by value_upper over the rest keeps its first element when that is NaN, and a later NaN never wins.
// Every index handed back is in [0, k), whatever the values are.
__device__ inline void gape_bai(const double *C, int k, int lane, int *selected, int *best, int *challenger)
{
    double top1, top2;
    const int i1 = gape_first_max(k, lane, 0, [&](int i) { return C[2 * i]; }, &top1);
    gape_first_max(k, lane, 0, [&](int i) { return i == i1 ? -INFINITY : C[2 * i]; }, &top2);
    const int b = gape_first_max(k, lane, 0, [&](int i) {
        const double gap = (i == i1 ? top2 : top1) - C[2 * i + 1];
        return isnan(gap) ? (double)INFINITY : -gap; // min by gap
    });
    const int rest0 = b == 0 ? 1 : 0; // the first of the rest (k >= 2)
    int c = rest0;
    if (!isnan(C[2 * rest0])) c = gape_first_max(k, lane, rest0, [&](int i) { return i == b ? -INFINITY : C[2 * i]; });
    const double wb = C[2 * b] - C[2 * b + 1], wc = C[2 * c] - C[2 * c + 1];
    *best = b; *challenger = c; *selected = wc > wb ? c : b; // max([best, challenger], key=width): the first unless exceeded
}

// np.amax of column `which` of the children's values: NaN if any is NaN
__device__ __forceinline__ double gape_amax(const double *C, int k, int which, int lane)
{
    double m = -INFINITY;
    bool nan_seen = false;
    for (int i = lane; i < k; i += 64) {
        const double v = C[2 * i + which];
        if (isnan(v)) nan_seen = true;
        else if (v > m) m = v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    return __ballot(nan_seen) ? (double)NAN : m;
}

// random_argmax over the children's value_upper (abstract.py:296-311): the positions equal to the maximum, one of them drawn by
// Generator.choice -- which draws nothing from a set of one.  -1 for an empty set (a NaN among the values: nothing equals the
// NaN np.amax returns, and Generator.choice raises ValueError), else a position in [0, k)
__device__ inline int gape_random_argmax(const double *C, int k, int lane, Pcg64 &gen)
{
    const double m = gape_amax(C, k, 0, lane);
    int ties = 0;
    for (int i0 = 0; i0 < k; i0 += 64) {
        const int i = i0 + lane;
        ties += __popcll(__ballot(i < k && C[2 * i] == m));
    }
    if (ties == 0) return -1;
    int r = ties > 1 ? (int)gen.below((uint32_t)ties) : 0;
    for (int i0 = 0; i0 < k; i0 += 64) {
        const int i = i0 + lane;
        unsigned long long bal = __ballot(i < k && C[2 * i] == m);
        const int c = __popcll(bal);
        if (r >= c) { r -= c; continue; }
        for (; r > 0; --r) bal &= bal - 1;
        return i0 + __ffsll((long long)bal) - 1;
    }
    return 0; // (not reached: r < ties)
}

} // namespace mp
