// Stand-alone host check of the LDS-resident UCT forms' 16-bit transition tables (rl_agents_amd/csrc/uct_term_table.hpp): the
// NEXT table, whose bit 15 is terminal[next], and the SOURCE table, whose bit 15 is terminal[s] of the state a record leaves.
// Built with -fsanitize=address,undefined and run by tests/test_uct_lean_step_host.py.
//
// For every listed model both tables are filled into heap arrays of EXACTLY S * |A| words (a write past them is an ASan report)
// and compared, record by record, with a restatement that never forms a word: a walk that leaves state s by action a stops under
// the rule "next" iff terminal[T[s][a]], under the rule "source" iff terminal[s], and moves to T[s][a] under both.  Then the
// property the kernel's step relies on: along walks from every state, the bit of the SOURCE table at step k is the bit of the NEXT
// table at step k - 1 (the `cur_term` a kernel without the second table carries), and terminal[root] at step 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rl_agents_amd/csrc/uct_term_table.hpp"

struct Model {
    const char *name;
    int S, A;
    std::vector<int32_t> T;
    std::vector<uint8_t> term;   // empty: the model was loaded without terminal flags
};

static int fails = 0;
static long records = 0, steps = 0;

static uint64_t lcg(uint64_t &x) { x = x * 6364136223846793005ULL + 1442695040888963407ULL; return x >> 33; }

static Model random_model(const char *name, int S, int A, uint64_t seed, int term_one_in, bool flags)
{
    Model m{name, S, A, std::vector<int32_t>((size_t)S * A), {}};
    uint64_t x = seed;
    for (auto &t : m.T) t = (int32_t)(lcg(x) % (uint64_t)S);
    if (flags) {
        m.term.assign((size_t)S, 0);
        for (auto &f : m.term) f = term_one_in > 0 && lcg(x) % (uint64_t)term_one_in == 0 ? 1 : 0;
    }
    return m;
}

static void check_model(const Model &m)
{
    const size_t n = (size_t)m.S * m.A;
    const uint8_t *term = m.term.empty() ? nullptr : m.term.data();
    uint16_t *next_tab = new uint16_t[n], *src_tab = new uint16_t[n];
    std::memset(next_tab, 0xa5, n * 2);
    std::memset(src_tab, 0x5a, n * 2);
    mp::uct_term_table_fill(m.S, m.A, m.T.data(), term, false, next_tab);
    mp::uct_term_table_fill(m.S, m.A, m.T.data(), term, true, src_tab);
    for (int s = 0; s < m.S; ++s)
        for (int a = 0; a < m.A; ++a) {
            const size_t i = (size_t)s * m.A + a;
            const int32_t nx = m.T[i];
            const bool stop_next = term && term[nx], stop_source = term && term[s];
            ++records;
            if ((next_tab[i] & 0x7fff) != nx || (src_tab[i] & 0x7fff) != nx) {
                std::printf("FAIL: %s: record (%d, %d): next state %d, tables hold %d and %d\n", m.name, s, a, nx, next_tab[i] & 0x7fff,
                            src_tab[i] & 0x7fff);
                ++fails;
            }
            if (((next_tab[i] >> 15) != 0) != stop_next) { std::printf("FAIL: %s: record (%d, %d): bit 15 of the next table\n", m.name, s, a); ++fails; }
            if (((src_tab[i] >> 15) != 0) != stop_source) { std::printf("FAIL: %s: record (%d, %d): bit 15 of the source table\n", m.name, s, a); ++fails; }
            // the per-record function, as the update kernels call it
            if (mp::uct_term_word(nx, stop_source, stop_next, false) != next_tab[i] || mp::uct_term_word(nx, stop_source, stop_next, true) != src_tab[i]) {
                std::printf("FAIL: %s: record (%d, %d): uct_term_word differs from the filled tables\n", m.name, s, a);
                ++fails;
            }
        }
    // walks: the carried bit against the source table
    uint64_t x = 12345;
    for (int s0 = 0; s0 < m.S; ++s0) {
        int s = s0;
        bool cur_term = term && term[s0];   // root_term
        for (int k = 0; k < 12; ++k) {
            const int a = (int)(lcg(x) % (uint64_t)m.A);
            const size_t i = (size_t)s * m.A + a;
            ++steps;
            if (((src_tab[i] >> 15) != 0) != cur_term) {
                std::printf("FAIL: %s: walk from %d, step %d: the source table's bit is not the carried one\n", m.name, s0, k);
                ++fails;
            }
            cur_term = (next_tab[i] >> 15) != 0;
            s = next_tab[i] & 0x7fff;
        }
    }
    delete[] next_tab;
    delete[] src_tab;
}

int main()
{
    std::vector<Model> models;
    models.push_back(random_model("random 23 x 5", 23, 5, 1, 6, true));
    models.push_back(random_model("random 40 x 2", 40, 2, 2, 3, true));
    models.push_back(random_model("every state terminal", 9, 3, 3, 1, true));
    models.push_back(random_model("no state terminal", 9, 3, 4, 0, true));
    models.push_back(random_model("no flags", 17, 6, 5, 0, false));
    models.push_back(random_model("one state", 1, 4, 6, 2, true));
    models.push_back(random_model("32 767 states (bit 14 set)", 32767, 2, 7, 5, true));
    {   // a terminal state whose successors are not, and a live state whose successors all are: the two tables differ in every record
        Model m{"swapped", 4, 2, {1, 1, 0, 0, 3, 3, 2, 2}, {1, 0, 0, 1}};
        models.push_back(m);
    }
    for (const Model &m : models) check_model(m);
    // "swapped": state 0 terminal -> 1 live; state 1 live -> 0 terminal; state 2 live -> 3 terminal; state 3 terminal -> 2 live
    {
        uint16_t a[8], b[8];
        const Model &m = models.back();
        mp::uct_term_table_fill(m.S, m.A, m.T.data(), m.term.data(), false, a);
        mp::uct_term_table_fill(m.S, m.A, m.T.data(), m.term.data(), true, b);
        for (int i = 0; i < 8; ++i)
            if (((a[i] ^ b[i]) & 0x8000) == 0) { std::printf("FAIL: swapped: record %d has the same bit in both tables\n", i); ++fails; }
    }
    if (fails) return 1;
    std::printf("ok: %zu models, %ld records, %ld walk steps\n", models.size(), records, steps);
    return 0;
}
