// Stand-alone host check of the rollout's action table (rl_agents_amd/csrc/uct_action_table.hpp): the byte per bucket of the
// draw's top twelve bits that uct_kernel's saturated form reads in place of the exact compares.  Built with
// -fsanitize=address,undefined and run by tests/test_uct_action_table_host.py.
//
// For every listed policy the thresholds are computed as the library computes them (uct_tables and uct_args_model: cumulative sum,
// ceil(cdf / sum * 2^53), shifted up by 11 bits, ~0 for those no draw reaches, thr_valid = how many of the first |A| - 1 are
// real), the table is filled into a heap array of EXACTLY kUctActBytes (a write past it is an ASan report), and at both ends of
// every bucket, at every threshold and one below and above it, at 0 and at 2^64 - 1 the entry must be the action that the
// restated rule gives -- t = min(#{a < |A| - 1 : thr_arg[a] <= x}, thr_valid) -- or kUctActExact; at most |A| - 1 entries may be
// kUctActExact.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rl_agents_amd/csrc/uct_action_table.hpp"

using mp::kUctActBits;
using mp::kUctActBytes;
using mp::kUctActExact;

struct Policy {
    const char *name;
    std::vector<double> p;
};

struct Thresholds {
    uint64_t arg[8];
    int valid;
};

static Thresholds thresholds(const std::vector<double> &p)
{
    const int A = (int)p.size();
    std::vector<double> cdf((size_t)A);
    double acc = 0.0;
    for (int a = 0; a < A; ++a) { acc += p[(size_t)a]; cdf[(size_t)a] = acc; }
    Thresholds t;
    t.valid = 0;
    for (int i = 0; i < 8; ++i) {
        t.arg[i] = ~0ULL;
        if (i >= A) continue;
        const double scaled = std::ceil(std::ldexp(cdf[(size_t)i] / acc, 53));
        const uint64_t k = scaled >= 18446744073709551615.0 ? ~0ULL : (uint64_t)scaled;
        if (k < (1ULL << 53)) {
            t.arg[i] = k << 11;
            if (i < A - 1) t.valid = i + 1;
        }
    }
    return t;
}

static int restated(const Thresholds &t, int nth, uint64_t x)
{
    int n = 0;
    for (int a = 0; a < nth; ++a)
        if (t.arg[a] <= x) ++n;
    return n < t.valid ? n : t.valid;
}

static int fails = 0;
static long points = 0;

static void check_point(const Policy &pol, const Thresholds &t, int nth, const uint8_t *tab, uint64_t x)
{
    const int want = restated(t, nth, x);
    const uint8_t got = tab[x >> (64 - kUctActBits)];
    ++points;
    if (mp::uct_action_exact(t.arg, nth, t.valid, x) != want) {
        std::printf("FAIL: %s: uct_action_exact(%016llx) differs from the restated rule (%d)\n", pol.name, (unsigned long long)x, want);
        ++fails;
    }
    if (got != kUctActExact && got != (uint8_t)want) {
        std::printf("FAIL: %s: draw %016llx: entry %d, action %d\n", pol.name, (unsigned long long)x, (int)got, want);
        ++fails;
    }
}

// -> the number of kUctActExact entries
static int check_policy(const Policy &pol)
{
    const int nth = (int)pol.p.size() - 1;
    const Thresholds t = thresholds(pol.p);
    uint8_t *tab = new uint8_t[kUctActBytes];
    std::memset(tab, 0xa5, kUctActBytes);
    const int reported = mp::uct_action_table_fill(t.arg, nth, t.valid, tab);
    int exact = 0;
    for (int b = 0; b < kUctActBytes; ++b) {
        exact += tab[b] == kUctActExact ? 1 : 0;
        if (tab[b] != kUctActExact && tab[b] > nth) { std::printf("FAIL: %s: bucket %d holds %d\n", pol.name, b, (int)tab[b]); ++fails; }
        const uint64_t lo = (uint64_t)b << (64 - kUctActBits), hi = lo | ((1ULL << (64 - kUctActBits)) - 1);
        check_point(pol, t, nth, tab, lo);
        check_point(pol, t, nth, tab, hi);
    }
    for (int a = 0; a < nth; ++a) {
        const uint64_t x = t.arg[a];
        check_point(pol, t, nth, tab, x);
        if (x > 0) check_point(pol, t, nth, tab, x - 1);
        if (x < ~0ULL) check_point(pol, t, nth, tab, x + 1);
    }
    check_point(pol, t, nth, tab, 0);
    check_point(pol, t, nth, tab, ~0ULL);
    if (exact != reported) { std::printf("FAIL: %s: %d exact entries, %d reported\n", pol.name, exact, reported); ++fails; }
    if (exact > nth) { std::printf("FAIL: %s: %d exact entries for %d thresholds\n", pol.name, exact, nth); ++fails; }
    delete[] tab;
    return exact;
}

int main()
{
    std::vector<Policy> policies;
    for (int k : {2, 3, 4, 5, 6, 8}) {
        static char names[9][16];
        std::snprintf(names[k], sizeof(names[k]), "uniform%d", k);
        policies.push_back({names[k], std::vector<double>((size_t)k, 1.0 / k)});
    }
    // two thresholds inside bucket 1024 (0.25 + 2^-14 and 0.25 + 2^-13: a bucket is 2^-12 wide)
    policies.push_back({"two in one bucket", {0.25 + 0x1p-14, 0x1p-14, 0.25, 0.5 - 0x1p-13}});
    policies.push_back({"a zero in the middle", {0.25, 0.0, 0.5, 0.25}});
    policies.push_back({"trailing zeros", {0.25, 0.0, 0.5, 0.25, 0.0, 0.0}});
    policies.push_back({"one action takes all", {0.0, 0.0, 1.0, 0.0, 0.0}});
    policies.push_back({"the first action takes all", {1.0, 0.0, 0.0}});
    long exact_total = 0;
    for (const Policy &pol : policies) {
        const int exact = check_policy(pol);
        exact_total += exact;
        if (!std::strcmp(pol.name, "two in one bucket")) {
            const Thresholds t = thresholds(pol.p);
            if ((t.arg[0] >> 52) != 1024 || (t.arg[1] >> 52) != 1024 || t.arg[0] == t.arg[1]) {
                std::printf("FAIL: the two thresholds do not share bucket 1024\n");
                ++fails;
            }
            // (the third threshold, 0.5 + 2^-13, lies in the middle of bucket 2048)
            if (exact != 2) { std::printf("FAIL: two in one bucket: %d exact entries, expected 2\n", exact); ++fails; }
        }
        // uniform5's thresholds (k / 5) all lie inside buckets: four exact entries
        if (!std::strcmp(pol.name, "uniform5") && exact != 4) { std::printf("FAIL: uniform5: %d exact entries, expected 4\n", exact); ++fails; }
        // thresholds on bucket boundaries need no exact entry: uniform2, 4 and 8
        if ((!std::strcmp(pol.name, "uniform2") || !std::strcmp(pol.name, "uniform4") || !std::strcmp(pol.name, "uniform8")) && exact != 0) {
            std::printf("FAIL: %s: %d exact entries, expected none\n", pol.name, exact);
            ++fails;
        }
    }
    if (fails) return 1;
    std::printf("ok: %zu policies, %ld points, %ld exact entries\n", policies.size(), points, exact_total);
    return 0;
}
