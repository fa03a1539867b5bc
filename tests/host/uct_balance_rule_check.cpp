// Stand-alone host check of the wave-balance rule (rl_agents_amd/csrc/uct_balance.hpp): the priority a wave of uct_kernel's
// saturated form runs its next rollout at, given the progress words of its workgroup.  Built with -fsanitize=address,undefined and
// run by tests/test_uct_balance_rule_host.py.
//
// The named cases (no mates, a finished mate, a tie, behind, ahead), then every workgroup size 1, 2, 4, 8, 16 under random
// placements and episodes against a restatement that is written from the sentence, not from the code: "priority 1 if some other
// planning wave sits on my SIMD and none of those is in an earlier episode than I am, else 0".  The word arrays have EXACTLY
// n_waves elements on the heap: a read past the workgroup's waves is an ASan report.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../rl_agents_amd/csrc/uct_balance.hpp"

using mp::kUctBalGone;
using mp::uct_bal_word;

struct Wave {
    bool planning;
    int episode;
    unsigned simd;
};

static int restated(const std::vector<Wave> &w, int me)
{
    int mates = 0;
    for (int i = 0; i < (int)w.size(); ++i) {
        if (i == me || !w[i].planning || w[i].simd != w[me].simd) continue;
        ++mates;
        if (w[i].episode < w[me].episode) return 0;
    }
    return mates > 0 ? 1 : 0;
}

static int by_rule(const std::vector<Wave> &w, int me)
{
    uint32_t *words = new uint32_t[w.size()];
    for (size_t i = 0; i < w.size(); ++i) words[i] = w[i].planning ? uct_bal_word(w[i].episode, w[i].simd) : kUctBalGone;
    const int p = mp::uct_rollout_prio(words, (int)w.size(), me);
    delete[] words;
    return p;
}

static int fails = 0;
static void expect(const char *what, const std::vector<Wave> &w, int me, int want)
{
    const int got = by_rule(w, me);
    if (got != want || restated(w, me) != want) {
        std::printf("FAIL: %s: priority %d (restatement %d), expected %d\n", what, got, restated(w, me), want);
        ++fails;
    }
}

int main()
{
    // ---- the named cases; wave 0 is "me", on SIMD 2 in episode 7
    expect("a lone wave", {{true, 7, 2}}, 0, 0);
    expect("no mates: the others sit on other SIMDs", {{true, 7, 2}, {true, 1, 0}, {true, 30, 1}, {true, 7, 3}}, 0, 0);
    expect("a finished mate only", {{true, 7, 2}, {false, 0, 2}}, 0, 0);
    expect("a finished mate and one that is ahead", {{true, 7, 2}, {false, 0, 2}, {true, 9, 2}}, 0, 1);
    expect("a tie", {{true, 7, 2}, {true, 7, 2}}, 0, 1);
    expect("a tie, seen from the other wave", {{true, 7, 2}, {true, 7, 2}}, 1, 1);
    expect("behind my mate", {{true, 7, 2}, {true, 8, 2}}, 0, 1);
    expect("ahead of my mate", {{true, 7, 2}, {true, 6, 2}}, 0, 0);
    expect("ahead of one mate, behind another", {{true, 7, 2}, {true, 6, 2}, {true, 20, 2}}, 0, 0);
    expect("ahead of a wave on another SIMD only", {{true, 7, 2}, {true, 6, 1}, {true, 7, 2}}, 0, 1);
    expect("episode 0 against episode 0", {{true, 0, 0}, {true, 0, 0}, {true, 0, 0}, {true, 0, 0}}, 3, 1);
    expect("the last episode of a long plan", {{true, (1 << 29) - 1, 3}, {true, (1 << 29) - 2, 3}}, 0, 0);
    // a finished wave is never a planning word: the largest episode with SIMD 3 still differs from it
    if (uct_bal_word((1 << 30) - 2, 3) == kUctBalGone) { std::printf("FAIL: a planning word equals the finished one\n"); ++fails; }

    // ---- every workgroup size, random placements (any the dispatcher may choose: all on one SIMD, none shared, ...) and episodes
    std::mt19937 g(20241020u);
    long cases = 0, raised = 0;
    for (int n_waves : {1, 2, 4, 8, 16}) {
        for (int rep = 0; rep < 4000; ++rep) {
            std::vector<Wave> w((size_t)n_waves);
            const unsigned simds = 1u + g() % 4u, spread = 1u + g() % 5u;
            for (Wave &x : w) x = Wave{g() % 5u != 0u, (int)(g() % spread) + (int)(g() % 30u == 0u ? g() % 1000u : 0u), (unsigned)(g() % simds)};
            for (int me = 0; me < n_waves; ++me) {
                if (!w[me].planning) continue;
                const int want = restated(w, me), got = by_rule(w, me);
                if (got != want) {
                    std::printf("FAIL: %d waves, rep %d, wave %d: priority %d, expected %d\n", n_waves, rep, me, got, want);
                    return 1;
                }
                ++cases;
                raised += got;
            }
        }
    }
    // among the planning waves of one SIMD the ones in the earliest episode are raised, nobody else (so somebody always runs at
    // the higher priority while two of them plan, and never everybody unless they are level)
    for (int rep = 0; rep < 2000; ++rep) {
        std::vector<Wave> w(4);
        for (Wave &x : w) x = Wave{true, (int)(g() % 4u), 1u};
        int lo = w[0].episode;
        for (const Wave &x : w) lo = x.episode < lo ? x.episode : lo;
        for (int me = 0; me < 4; ++me)
            if (by_rule(w, me) != (w[me].episode == lo ? 1 : 0)) { std::printf("FAIL: four mates, rep %d, wave %d\n", rep, me); return 1; }
    }
    if (fails) return 1;
    if (raised < cases / 20 || raised > cases - cases / 20) { std::printf("FAIL: %ld of %ld cases raised: the cases are one-sided\n", raised, cases); return 1; }
    std::printf("ok: %ld cases, %ld at priority 1\n", cases, raised);
    return 0;
}
