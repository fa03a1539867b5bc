// uct_term_table.hpp -- the 16-bit transition tables of the LDS-resident UCT forms: {bit 15: a terminal flag, bits 0-14: next
// state}, one word per (s, a), for models of fewer than 32 768 states.  Plain C++ outside a HIP compilation: api.hip (the load and
// the update kernels) and a stand-alone host test include it.
//
// THE BIT'S TWO MEANINGS.  An env step of a table model stops on terminal[next] with done_on_next and on terminal[s] of the state
// it leaves without it (trainer/evaluation.py's two loops).  The flag is a function of the state -- a model is loaded with
// terminal[S], nothing per action -- so either rule can be written into the record a step reads anyway:
//   * the NEXT table (mp_model::t16) carries terminal[next].  Every LDS form stages it for done_on_next; the four-lane form,
//     uct_lone_kernel and uct_row_kernel stage it for both rules and carry the bit one step for the other;
//   * the SOURCE table (mp_model::t16s) carries terminal[s].  uct_kernel's one-lane LDS-resident form stages it for models
//     without done_on_next, and its step tests bit 15 under either rule (uct.hip, THE LEAN TRIP).
// Bits 0-14 are the same in both.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MP_TERM_TABLE_FN __host__ __device__ inline
#else
#define MP_TERM_TABLE_FN inline
#endif

namespace mp {

// the word of (s, a) -> next: `source` chooses the table
MP_TERM_TABLE_FN uint16_t uct_term_word(int32_t next, bool term_s, bool term_next, bool source)
{
    return (uint16_t)((uint32_t)next | ((source ? term_s : term_next) ? 0x8000u : 0u));
}

// One table of a whole model on the host: T[S * A] next states in [0, S), S < 32 768; term[S] or nullptr (no terminal state).
inline void uct_term_table_fill(int S, int A, const int32_t *T, const uint8_t *term, bool source, uint16_t *out)
{
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < A; ++a) {
            const int32_t nx = T[(long)s * A + a];
            out[(long)s * A + a] = uct_term_word(nx, term && term[s], term && term[nx], source);
        }
}

} // namespace mp
