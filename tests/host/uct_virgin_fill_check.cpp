// Stand-alone host check of uct_virgin_fill (rl_agents_amd/csrc/uct_virgin.hpp), the export's reading of UCT trees whose virgin
// groups were never stored.  Built with -fsanitize=address,undefined and run by tests/test_uct_virgin_fill_host.py.
//
// Synthetic trees: random trees grown the way a plan grows them (a node expands on its first visit, a later visit descends),
// node arrays of EXACTLY `cap` elements on the heap (a write past the end is an ASan report), the children of every count-1 node
// overwritten with garbage -- first_child values far outside the array included.  The fill must restore the complete tree and
// return its size; a plain restatement (recursive, from the root) says what the complete tree is.  With virgin == false the
// function must change nothing and follow the links as they are.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../rl_agents_amd/csrc/uct_virgin.hpp"

struct Node {
    double value;
    int32_t count;
    int32_t first_child;
};

static bool same(const Node &a, const Node &b)
{
    return std::memcmp(&a.value, &b.value, sizeof(double)) == 0 && a.count == b.count && a.first_child == b.first_child;
}

// a complete tree of `episodes` visits from the root: every visit walks random children to a node without children, which expands
// unless it is at depth `horizon`, and adds one to the counts on its way
static std::vector<Node> grow(std::mt19937 &g, int A, int episodes, int horizon, int cap)
{
    std::vector<Node> t(1, Node{0.0, 0, -1});
    for (int e = 0; e < episodes; ++e) {
        int node = 0, depth = 0;
        std::vector<int> path(1, 0);
        while (t[node].first_child >= 0 && depth < horizon) {
            node = t[node].first_child + (int)(g() % (unsigned)A);
            path.push_back(node);
            ++depth;
        }
        if (t[node].first_child < 0 && depth < horizon && (int)t.size() + A <= cap) {
            t[node].first_child = (int)t.size();
            for (int a = 0; a < A; ++a) t.push_back(Node{0.0, 0, -1});
        }
        for (int n : path) { t[n].count += 1; t[n].value += 0.25 * (double)(g() % 7u); }
    }
    return t;
}

// the restatement: walk from the root, and below a count-1 node take the constant node instead of what the array holds
static void expect_from(const std::vector<Node> &stored, int A, int node, bool constant, std::vector<Node> &out, int &n)
{
    const Node me = constant ? Node{0.0, 0, -1} : stored[node];
    out[node] = me;
    if (me.first_child < 0) return;
    if (me.first_child + A > n) n = me.first_child + A;
    for (int a = 0; a < A; ++a) expect_from(stored, A, me.first_child + a, me.count == 1, out, n);
}

int main()
{
    std::mt19937 g(20240607u);
    int trees = 0, groups = 0;
    for (int rep = 0; rep < 400; ++rep) {
        const int A = 2 + (int)(g() % 7u), episodes = 1 + (int)(g() % 60u), horizon = 1 + (int)(g() % 9u);
        const int cap = 1 + episodes * A;
        const std::vector<Node> whole = grow(g, A, episodes, horizon, cap);
        // the device array: cap elements, garbage behind the tree and in the groups below count-1 nodes
        Node *h = new Node[cap];
        for (int i = 0; i < cap; ++i) h[i] = Node{-1.5, (int32_t)(g() % 1000u) - 3, (int32_t)(g() % 4000000u) - 100};
        for (size_t i = 0; i < whole.size(); ++i) h[i] = whole[i];
        for (size_t i = 0; i < whole.size(); ++i)
            if (whole[i].count == 1 && whole[i].first_child >= 0) {
                ++groups;
                for (int a = 0; a < A; ++a) h[whole[i].first_child + a] = Node{7.0, 1 + (int32_t)(g() % 9u), (int32_t)(g() % 100000u)};
            }
        const std::vector<Node> stored(h, h + cap);
        std::vector<Node> want(stored);
        int n_want = 1;
        expect_from(stored, A, 0, false, want, n_want);
        const int n = mp::uct_virgin_fill(h, cap, A, true);
        if (n != n_want || n != (int)whole.size()) { std::printf("FAIL: size %d, expected %d = %d (rep %d)\n", n, n_want, (int)whole.size(), rep); return 1; }
        for (int i = 0; i < cap; ++i)
            if (!same(h[i], want[i])) { std::printf("FAIL: node %d of rep %d\n", i, rep); return 1; }
        for (int i = 0; i < n; ++i)
            if (!same(h[i], whole[i])) { std::printf("FAIL: node %d of rep %d is not the complete tree's\n", i, rep); return 1; }
        // virgin == false: nothing is written, and a complete tree gives the same size
        Node *c = new Node[cap];
        for (int i = 0; i < cap; ++i) c[i] = h[i];
        const int n2 = mp::uct_virgin_fill(c, cap, A, false);
        if (n2 != n) { std::printf("FAIL: size %d of the complete tree, expected %d (rep %d)\n", n2, n, rep); return 1; }
        for (int i = 0; i < cap; ++i)
            if (!same(c[i], h[i])) { std::printf("FAIL: a complete tree was changed (rep %d)\n", rep); return 1; }
        delete[] c;
        delete[] h;
        ++trees;
    }
    // a count-1 node whose group would end past the array (a damaged tree): nothing is written outside it
    {
        Node *h = new Node[4];
        h[0] = Node{1.0, 1, 2};
        for (int i = 1; i < 4; ++i) h[i] = Node{3.0, 3, -1};
        (void)mp::uct_virgin_fill(h, 4, 5, true);
        if (!(h[1].count == 3 && h[2].count == 0 && h[3].count == 0)) { std::printf("FAIL: the short array\n"); return 1; }
        delete[] h;
    }
    if (groups < 400) { std::printf("FAIL: only %d unstored groups in %d trees\n", groups, trees); return 1; }
    std::printf("ok: %d trees, %d unstored groups\n", trees, groups);
    return 0;
}
