// Stand-alone host check of Pcg64W (rl_agents_amd/csrc/pcg64.hpp: the PCG64 step on four 32-bit words), the header's host path
// against unsigned __int128.  Built with -fsanitize=address,undefined and run by tests/test_pcg64_words_host.py, which hands
// over the case list of tests/pcg64_words_cases.py as a file of lines "s_hi s_lo inc_hi inc_lo" (hex); a few million random
// records follow.  Every record: from() / state_to() round trip, three steps, and the output of each state.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../rl_agents_amd/csrc/pcg64.hpp"

typedef unsigned __int128 u128;

struct Halves {                 // what Pcg64W::from / state_to expect of a generator: Pcg64's four members
    uint64_t s_hi, s_lo, inc_hi, inc_lo;
};

static const u128 MULT = ((u128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL;

static uint64_t output128(u128 s)
{
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s, x = hi ^ lo;
    const unsigned r = (unsigned)(hi >> 58);
    return (x >> r) | (x << ((64u - r) & 63u));
}

static int check(const Halves &h, const char *what, long idx)
{
    mp::Pcg64W w = mp::Pcg64W::from(h);
    Halves back = h;
    back.s_hi = back.s_lo = 0;
    w.state_to(back);
    if (back.s_hi != h.s_hi || back.s_lo != h.s_lo) {
        std::printf("FAIL %s %ld: from / state_to round trip\n", what, idx);
        return 1;
    }
    u128 s = ((u128)h.s_hi << 64) | h.s_lo;
    const u128 inc = ((u128)h.inc_hi << 64) | h.inc_lo;
    for (int k = 0; k < 3; ++k) {
        uint32_t lo, hi;
        w.output(lo, hi);
        if ((((uint64_t)hi << 32) | lo) != output128(s)) {
            std::printf("FAIL %s %ld: output before step %d\n", what, idx, k);
            return 1;
        }
        s = s * MULT + inc;
        mp::Pcg64W v = w;
        const uint64_t n = v.next64();
        w.advance();
        Halves got = h;
        w.state_to(got);
        if (got.s_hi != (uint64_t)(s >> 64) || got.s_lo != (uint64_t)s || n != output128(s) || v.w3 != w.w3 || v.w0 != w.w0) {
            std::printf("FAIL %s %ld: step %d: %016" PRIx64 " %016" PRIx64 " want %016" PRIx64 " %016" PRIx64 "\n", what, idx, k,
                        got.s_hi, got.s_lo, (uint64_t)(s >> 64), (uint64_t)s);
            return 1;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    long n_cases = 0, n_random = argc > 2 ? std::atol(argv[2]) : 3000000;
    if (argc > 1) {
        std::FILE *f = std::fopen(argv[1], "r");
        if (!f) {
            std::printf("FAIL cannot open %s\n", argv[1]);
            return 2;
        }
        Halves h;
        while (std::fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &h.s_hi, &h.s_lo, &h.inc_hi, &h.inc_lo) == 4) {
            if (check(h, "case", n_cases)) return 1;
            ++n_cases;
        }
        std::fclose(f);
    }
    std::mt19937_64 g(20240607);
    for (long i = 0; i < n_random; ++i) {
        Halves h{g(), g(), g(), g() | 1ULL};
        if (i % 7 == 0) h.s_lo |= 0xffffffff00000000ULL;          // words of all ones, zeros: carries that random words rarely meet
        if (i % 11 == 0) h.inc_lo |= 0x00000000ffffffffULL;
        if (i % 13 == 0) h.s_hi &= 0xffffffffULL;
        if (check(h, "random", i)) return 1;
    }
    std::printf("ok: %ld cases, %ld random records\n", n_cases, n_random);
    return 0;
}
