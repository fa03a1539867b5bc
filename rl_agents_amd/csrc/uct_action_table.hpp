// uct_action_table.hpp -- the rollout action of uct_kernel's saturated form (one-lane LDS-resident model, state-independent
// policies) as a byte table of DRAW BUCKETS.  Plain C++ (no HIP): the kernel, the launch code of uct.hip and a stand-alone host
// test include it.
//
// A rollout step picks its action as searchsorted(cdf, u, 'right') = min(#{a < NTH : thr_arg[a] <= draw}, thr_valid) on the raw
// 64-bit draw (thr_arg, thr_valid: UctArgs -- the thresholds shifted up by 11 bits, ~0 for those no draw reaches, and how many of
// them are real).  The count is monotone in the draw, so over the bucket of the 2^52 draws that share their top twelve bits it is
// constant unless a threshold lies inside the bucket above its first value -- at most NTH buckets of the 4 096, whatever the
// policy.  The table holds the action of every other bucket and kUctActExact for those: the kernel reads one byte per step and
// takes the exact compares only in a step where some lane of the wave meets kUctActExact (profiles/uct_action_table.md).
#pragma once

#include <cstdint>

namespace mp {

constexpr int kUctActBits = 12;                  // the draw's top bits that index the table
constexpr int kUctActBytes = 1 << kUctActBits;   // what the launch adds to the dynamic LDS, behind the balance words
constexpr uint8_t kUctActExact = 0xff;           // this bucket holds a threshold: the exact compares decide

// The instantiations of uct_kernel<AT, ENV, SP, MK, IL, QD> that take the table: the one-lane LDS-resident form (ENV 3) of the
// |A| that gain no register spill and no scratch and keep their waves per SIMD with it (profiles/uct_action_table_resources.txt).
// |A| = 7 and 8 spill already and would spill more: they run as before.
constexpr bool uct_action_table_form(int AT, int ENV, bool SP, bool MK, int IL, bool QD)
{
    return ENV == 3 && IL == 2 && !SP && !MK && !QD && AT >= 2 && AT <= 6;
}

// the action of a draw by the exact compares: what the table abbreviates
inline int uct_action_exact(const uint64_t *thr_arg, int nth, int thr_valid, uint64_t draw)
{
    int act = 0;
    for (int a = 0; a < nth; ++a) act += thr_arg[a] <= draw ? 1 : 0;
    return act < thr_valid ? act : thr_valid;
}

// Fills tab[0 .. kUctActBytes) from the first `nth` thresholds (nth = |A| - 1 <= 7) and returns how many entries are
// kUctActExact (<= nth).  Bucket b covers the draws lo = b << 52 .. hi = lo | (2^52 - 1): its entry is the action at lo if the
// action at hi is the same, kUctActExact otherwise.
inline int uct_action_table_fill(const uint64_t *thr_arg, int nth, int thr_valid, uint8_t *tab)
{
    int exact = 0;
    for (int b = 0; b < kUctActBytes; ++b) {
        const uint64_t lo = (uint64_t)b << (64 - kUctActBits), hi = lo | ((1ULL << (64 - kUctActBits)) - 1);
        const int at_lo = uct_action_exact(thr_arg, nth, thr_valid, lo), at_hi = uct_action_exact(thr_arg, nth, thr_valid, hi);
        tab[b] = at_lo == at_hi ? (uint8_t)at_lo : kUctActExact;
        exact += at_lo == at_hi ? 0 : 1;
    }
    return exact;
}

} // namespace mp
