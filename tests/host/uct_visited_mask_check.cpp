// Stand-alone host check of the visited-mask rule of rl_agents_amd/csrc/uct_virgin.hpp: the first_child word of an expanded node is
// first_child | mask << 24, bit a of the mask says that child a was stored, and a child whose bit is clear is {0.0, 0, -1} whatever
// its memory holds.  uct_virgin_fill(.., kUctTreeMasked) must make such a tree whole -- plain words, the constant below clear
// bits -- and return its size; the word helpers must strip and test as the rule says.  Built with -fsanitize=address,undefined
// and run by tests/test_uct_visited_mask_host.py.
//
// Hand-made trees: mask 0, the full mask, a clear bit over garbage memory, -1 words, a first_child of 2^24 - 1 (in an array that
// really holds that node, and in one that is too short for it).  Random trees grown the way a plan grows them, node arrays of
// EXACTLY `cap` elements on the heap, every node no visit reached overwritten with garbage; a plain restatement (recursive, from
// the root) says what the whole tree is.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../rl_agents_amd/csrc/uct_virgin.hpp"

struct Node {
    double value;
    int32_t count;
    int32_t first_child;
};

static const Node kConstant = {0.0, 0, -1};
static const Node kGarbage = {7.5, 12, 0x05000031};

static bool same(const Node &a, const Node &b)
{
    return std::memcmp(&a.value, &b.value, sizeof(double)) == 0 && a.count == b.count && a.first_child == b.first_child;
}

#define CHECK(cond, what)                                     \
    do {                                                      \
        if (!(cond)) { std::printf("FAIL: %s\n", what); return 1; } \
    } while (0)

// the restatement: the word's low 24 bits are the first child, bit 24 + a says whether child a is what the array holds
static void expect_from(const std::vector<Node> &stored, int A, int node, bool constant, std::vector<Node> &out, int &n)
{
    Node me = constant ? kConstant : stored[node];
    const int word = me.first_child;
    if (word >= 0) me.first_child = word % (1 << 24);
    out[node] = me;
    if (word < 0) return;
    if (me.first_child + A > n) n = me.first_child + A;
    for (int a = 0; a < A; ++a) expect_from(stored, A, me.first_child + a, ((word >> 24) >> a) % 2 == 0, out, n);
}

// a whole tree of `episodes` visits and, per node, which of its children a visit picked
static std::vector<Node> grow(std::mt19937 &g, int A, int episodes, int horizon, int cap, std::vector<unsigned> &picked)
{
    std::vector<Node> t(1, kConstant);
    picked.assign(1, 0u);
    for (int e = 0; e < episodes; ++e) {
        int node = 0, depth = 0;
        std::vector<int> path(1, 0);
        while (t[node].first_child >= 0 && depth < horizon) {
            const int a = (int)(g() % (unsigned)A);
            picked[node] |= 1u << a;
            node = t[node].first_child + a;
            path.push_back(node);
            ++depth;
        }
        if (t[node].first_child < 0 && depth < horizon && (int)t.size() + A <= cap) {
            t[node].first_child = (int)t.size();
            for (int a = 0; a < A; ++a) { t.push_back(kConstant); picked.push_back(0u); }
        }
        for (int n : path) { t[n].count += 1; t[n].value += 0.25 * (double)(g() % 7u); }
    }
    return t;
}

int main()
{
    // ---- the word helpers
    CHECK(mp::uct_word_child(-1) == -1 && mp::uct_word_mask(-1) == 0u && !mp::uct_word_stored(-1, 0), "-1 stays -1 and has no stored child");
    CHECK(mp::uct_word_child(6) == 6 && mp::uct_word_mask(6) == 0u, "mask 0");
    CHECK(mp::uct_word_child(6 | (0x1f << 24)) == 6 && mp::uct_word_mask(6 | (0x1f << 24)) == 0x1fu, "the full mask of five children");
    CHECK(mp::uct_word_child(0xffffff | (0x0a << 24)) == 0xffffff && mp::uct_word_mask(0xffffff | (0x0a << 24)) == 0x0au,
          "first_child 2^24 - 1");
    CHECK(mp::uct_word_stored(0xffffff | (0x0a << 24), 1) && !mp::uct_word_stored(0xffffff | (0x0a << 24), 2), "single bits");
    CHECK(mp::kUctChildBits == 0xffffff && mp::kUctMaskShift == 24, "the layout of the word");

    // ---- hand-made trees, |A| = 3: root 0, its children 1..3, the children of node 2 at 4..6
    {
        // mask 0 everywhere below the root: nothing below it was stored, garbage in every slot
        Node h[7] = {{2.0, 2, 1 | (0x2 << 24)}, kGarbage, {1.0, 1, 4}, kGarbage, kGarbage, kGarbage, kGarbage};
        const int n = mp::uct_virgin_fill(h, 7, 3, mp::kUctTreeMasked);
        CHECK(n == 7, "mask 0: size");
        CHECK(h[0].first_child == 1 && h[2].first_child == 4 && h[2].count == 1, "mask 0: plain words");
        for (int i : {1, 3, 4, 5, 6}) CHECK(same(h[i], kConstant), "mask 0: the constant below clear bits");
    }
    {
        // the full mask: every child is what the array holds
        Node h[7] = {{2.0, 5, 1 | (0x7 << 24)}, {0.5, 1, -1}, {1.0, 3, 4 | (0x7 << 24)}, {0.25, 1, -1}, {1.5, 1, -1}, {2.5, 1, -1}, {3.5, 1, -1}};
        const Node want[7] = {{2.0, 5, 1}, {0.5, 1, -1}, {1.0, 3, 4}, {0.25, 1, -1}, {1.5, 1, -1}, {2.5, 1, -1}, {3.5, 1, -1}};
        const int n = mp::uct_virgin_fill(h, 7, 3, mp::kUctTreeMasked);
        CHECK(n == 7, "full mask: size");
        for (int i = 0; i < 7; ++i) CHECK(same(h[i], want[i]), "full mask: nodes as stored, words plain");
    }
    {
        // a clear bit over garbage that looks like an expanded node far outside the array: it must not be followed
        Node h[7] = {{2.0, 4, 1 | (0x5 << 24)}, {0.5, 2, 4 | (0x4 << 24)}, {9.0, 9, 4000000}, {0.25, 1, -1}, kGarbage, {8.0, 3, 900}, {1.5, 1, -1}};
        const int n = mp::uct_virgin_fill(h, 7, 3, mp::kUctTreeMasked);
        CHECK(n == 7, "clear bit over garbage: size");
        CHECK(same(h[2], kConstant) && same(h[4], kConstant) && same(h[5], kConstant), "clear bit over garbage: the constant");
        CHECK(h[1].first_child == 4 && h[1].count == 2 && same(h[6], Node{1.5, 1, -1}) && same(h[3], Node{0.25, 1, -1}), "clear bit over garbage: the stored ones");
    }
    {
        // -1 words: a root that never expanded, and leaves
        Node a[1] = {{0.0, 0, -1}};
        CHECK(mp::uct_virgin_fill(a, 1, 3, mp::kUctTreeMasked) == 1 && same(a[0], kConstant), "-1 root");
        Node h[4] = {{1.0, 3, 1 | (0x7 << 24)}, {1.0, 1, -1}, {1.0, 1, -1}, {1.0, 1, -1}};
        CHECK(mp::uct_virgin_fill(h, 4, 3, mp::kUctTreeMasked) == 4 && h[1].first_child == -1 && h[3].first_child == -1, "-1 leaves");
    }
    {
        // first_child 2^24 - 1 in an array that holds the group (256 MB; every slot in between is a leaf, as the closure of the
        // links counts them all), bit 1 set
        const int fc = (1 << 24) - 1, A = 3, cap = fc + A;
        Node *h = static_cast<Node *>(std::malloc((size_t)cap * sizeof(Node)));
        CHECK(h != nullptr, "no memory for the 2^24-node array");
        for (int i = 0; i < cap; ++i) h[i] = kConstant;
        h[0] = Node{1.0, 2, fc | (0x2 << 24)};
        h[fc] = kGarbage; h[fc + 1] = Node{0.75, 1, -1}; h[fc + 2] = kGarbage;
        const int n = mp::uct_virgin_fill(h, cap, A, mp::kUctTreeMasked);
        CHECK(n == cap && h[0].first_child == fc, "first_child 2^24 - 1: size and word");
        CHECK(same(h[fc], kConstant) && same(h[fc + 1], Node{0.75, 1, -1}) && same(h[fc + 2], kConstant), "first_child 2^24 - 1: the group");
        std::free(h);
        // ... and in one that is too short for it (a damaged tree): nothing is written outside
        Node *s = new Node[2];
        s[0] = Node{1.0, 2, fc | (0x2 << 24)};
        s[1] = kGarbage;
        (void)mp::uct_virgin_fill(s, 2, A, mp::kUctTreeMasked);
        CHECK(s[0].first_child == fc && s[1].count == kGarbage.count && s[1].value == kGarbage.value, "first_child 2^24 - 1: the short array");
        delete[] s;
    }

    // ---- random trees
    std::mt19937 g(20240611u);
    int trees = 0, unstored = 0;
    for (int rep = 0; rep < 400; ++rep) {
        const int A = 2 + (int)(g() % 4u), episodes = 1 + (int)(g() % 60u), horizon = 1 + (int)(g() % 9u);
        const int cap = 1 + episodes * A;
        std::vector<unsigned> picked;
        const std::vector<Node> whole = grow(g, A, episodes, horizon, cap, picked);
        Node *h = new Node[cap];
        for (int i = 0; i < cap; ++i) h[i] = Node{-1.5, (int32_t)(g() % 1000u) - 3, (int32_t)(g() % 4000000u) - 100};
        for (size_t i = 0; i < whole.size(); ++i) h[i] = whole[i];
        for (size_t i = 0; i < whole.size(); ++i) {
            if (whole[i].first_child < 0) continue;
            h[i].first_child = whole[i].first_child | (int32_t)(picked[i] << 24);
            for (int a = 0; a < A; ++a)
                if (!((picked[i] >> a) & 1u)) {
                    ++unstored;
                    h[whole[i].first_child + a] = Node{7.0, 1 + (int32_t)(g() % 9u), (int32_t)(g() % 0x7fffffffu)};
                }
        }
        const std::vector<Node> stored(h, h + cap);
        std::vector<Node> want(stored);
        int n_want = 1;
        expect_from(stored, A, 0, false, want, n_want);
        const int n = mp::uct_virgin_fill(h, cap, A, mp::kUctTreeMasked);
        if (n != n_want || n != (int)whole.size()) { std::printf("FAIL: size %d, expected %d = %d (rep %d)\n", n, n_want, (int)whole.size(), rep); return 1; }
        for (int i = 0; i < cap; ++i)
            if (!same(h[i], want[i])) { std::printf("FAIL: node %d of rep %d\n", i, rep); return 1; }
        for (int i = 0; i < n; ++i)
            if (!same(h[i], whole[i])) { std::printf("FAIL: node %d of rep %d is not the whole tree's\n", i, rep); return 1; }
        // the whole tree read as a whole tree: nothing changes
        const std::vector<Node> before(h, h + cap);
        const int n2 = mp::uct_virgin_fill(h, cap, A, mp::kUctTreeWhole);
        if (n2 != n) { std::printf("FAIL: size %d of the whole tree, expected %d (rep %d)\n", n2, n, rep); return 1; }
        for (int i = 0; i < cap; ++i)
            if (!same(h[i], before[i])) { std::printf("FAIL: a whole tree was changed (rep %d)\n", rep); return 1; }
        delete[] h;
        ++trees;
    }
    if (unstored < 2000) { std::printf("FAIL: only %d unstored nodes in %d trees\n", unstored, trees); return 1; }
    std::printf("ok: %d trees, %d unstored nodes\n", trees, unstored);
    return 0;
}
