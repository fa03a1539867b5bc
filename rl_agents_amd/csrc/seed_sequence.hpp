// seed_sequence.hpp -- numpy.random.SeedSequence -> the six-word PCG64 record, on the host and on the device.
//
// numpy/random/bit_generator.pyx SeedSequence (pool of 4 uint32 words) and PCG64's seeding from generate_state(4, uint64),
// restated; tests/test_host_logic.py compares the records of the host entry points (mp_seed_sequence_states) with numpy's.
// The BRUE kernel (brue.hip) calls it once per rollout of a stochastic model: the reference re-seeds its env clone with
// state.seed(np_random.randint(2**30)) (brue.py:25), i.e. Generator(PCG64(SeedSequence(x))).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mp {

constexpr uint32_t kSsInitA = 0x43b0d7e5u, kSsMultA = 0x931e8875u, kSsInitB = 0x8b51f9ddu, kSsMultB = 0x58f38dedu;
constexpr uint32_t kSsMixL = 0xca01f9ddu, kSsMixR = 0x4973f715u;

__host__ __device__ inline uint32_t ss_hashmix(uint32_t value, uint32_t &hash_const)
{
    value ^= hash_const;
    hash_const *= kSsMultA;
    value *= hash_const;
    value ^= value >> 16;
    return value;
}
__host__ __device__ inline uint32_t ss_mix(uint32_t x, uint32_t y)
{
    uint32_t r = kSsMixL * x - kSsMixR * y;
    r ^= r >> 16;
    return r;
}
// entropy words (already split into uint32, no spawn key) -> the six-word PCG64 record
__host__ __device__ inline void seed_sequence_record(const uint32_t *entropy, int n, uint64_t *rec)
{
    uint32_t pool[4], hc = kSsInitA;
    for (int i = 0; i < 4; ++i) pool[i] = ss_hashmix(i < n ? entropy[i] : 0u, hc);
    for (int src = 0; src < 4; ++src)
        for (int dst = 0; dst < 4; ++dst)
            if (src != dst) pool[dst] = ss_mix(pool[dst], ss_hashmix(pool[src], hc));
    for (int src = 4; src < n; ++src)
        for (int dst = 0; dst < 4; ++dst) pool[dst] = ss_mix(pool[dst], ss_hashmix(entropy[src], hc));
    uint32_t w[8], hb = kSsInitB;
    for (int i = 0; i < 8; ++i) {          // generate_state(4, uint64) = 8 uint32 words viewed as 4 little-endian uint64
        uint32_t v = pool[i & 3];
        v ^= hb;
        hb *= kSsMultB;
        v *= hb;
        v ^= v >> 16;
        w[i] = v;
    }
    uint64_t q[4];
    for (int i = 0; i < 4; ++i) q[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    typedef unsigned __int128 u128;
    const u128 mult = ((u128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL;
    const u128 initstate = ((u128)q[0] << 64) | q[1], initseq = ((u128)q[2] << 64) | q[3];
    const u128 inc = (initseq << 1) | 1u;        // pcg_setseq_128_srandom_r
    u128 state = 0;
    state = state * mult + inc;
    state += initstate;
    state = state * mult + inc;
    rec[0] = (uint64_t)(state >> 64); rec[1] = (uint64_t)state;
    rec[2] = (uint64_t)(inc >> 64); rec[3] = (uint64_t)inc;
    rec[4] = 0; rec[5] = 0;                      // has_uint32, uinteger
}

} // namespace mp
