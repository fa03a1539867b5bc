// uct_balance.hpp -- the rule by which the waves of uct_kernel's saturated form (one-lane LDS-resident model: sixteen waves per
// workgroup, four per SIMD) keep level with the mates they share a SIMD with.  Plain C++ (no HIP): the kernel and a stand-alone
// host test include it.
//
// Every wave of a workgroup owns one PROGRESS WORD in LDS: `episode << 2 | SIMD_ID` while it plans, kUctBalGone once it has
// left (or if it never had a root).  The words are advisory: a wave only ever reads them to pick the priority of its next
// rollout, it never waits for one, and no result is computed from them (profiles/uct_wave_balance.md).
#pragma once

#include <cstdint>

namespace mp {

constexpr uint32_t kUctBalGone = 0xffffffffu;   // a wave that is not planning (any more): nobody's mate
constexpr int kUctBalWords = 16;                // one word per wave of the largest workgroup
constexpr int kUctBalBytes = kUctBalWords * 4;  // what the launch adds to the dynamic LDS behind the model

// The |A| whose one-lane LDS-resident kernel takes part: those that gain no register spill and no scratch and keep their waves
// per SIMD with the balance compiled in (profiles/uct_wave_balance.md).  |A| = 7 and 8 spill already and would spill more: they
// run as before.
constexpr bool uct_balance_form(int AT) { return AT >= 2 && AT <= 6; }

constexpr uint32_t uct_bal_word(int episode, uint32_t simd) { return ((uint32_t)episode << 2) | (simd & 3u); }

// Is the wave of `word` a mate of the wave of `mine` (another planning wave on the same SIMD) that is BEHIND it (in an earlier
// episode)?  The two words belong to different waves.
constexpr bool uct_bal_behind(uint32_t mine, uint32_t word)
{
    return word != kUctBalGone && ((word ^ mine) & 3u) == 0u && (word >> 2) < (mine >> 2);
}
constexpr bool uct_bal_mate(uint32_t mine, uint32_t word) { return word != kUctBalGone && ((word ^ mine) & 3u) == 0u; }

// The priority a wave runs its next rollout at: 1 while it has a planning mate and none of its mates is behind it -- it is (one
// of) the last on its SIMD, and the mates that are ahead drop to 0 and leave it the issue slots -- and 0 otherwise: a wave that is
// ahead of a mate, and a wave without mates (nothing to level: the schedule is what it was).  `words`: the progress words of the
// workgroup's `n_waves` waves, `me` this wave's index.
constexpr int uct_rollout_prio(const uint32_t *words, int n_waves, int me)
{
    bool mate = false;
    for (int w = 0; w < n_waves; ++w) {
        if (w == me) continue;
        if (uct_bal_behind(words[me], words[w])) return 0;
        mate = mate || uct_bal_mate(words[me], words[w]);
    }
    return mate ? 1 : 0;
}

} // namespace mp
