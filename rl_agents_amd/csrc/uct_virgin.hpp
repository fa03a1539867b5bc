// uct_virgin.hpp -- the rules that let uct_kernel leave zero nodes out of memory, for everything that reads its trees.  Plain C++
// (no HIP): the kernel, the host readers of uct.hip and a stand-alone host test include it.
//
// A UCT node expands on its FIRST visit only (mcts.py:151-154: the selection stops at a node without children, which then
// expands), and a later visit descends into one of the children and backs it up.  So in a tree without phantom slots
//     count == 1 and first_child >= 0   =>   the |A| children are all {value 0.0, count 0, first_child -1}
// (re-rooted trees included: a node that expands late there has count >= 2).  THE COUNT-1 RULE (kUctTreeCount1): a fresh-tree
// plan of a form that takes part (uct_virgin_form) with MP_UCT_TREE_STORES=virgin writes no such group: its memory holds whatever
// was there until the first entry completes it, and every reader substitutes the constant node below a count-1 node.
//
// THE VISITED MASK (kUctTreeMasked, the default of the forms of uct_mask_form) generalises it to the single child: a child that no
// episode has picked is the constant node as well, so only the picked ones are ever stored.  The first_child word of an expanded
// node is
//     first_child | mask << 24          bit a of mask set  <=>  the record of child a has been stored
// and a child whose bit is clear is {0.0, 0, -1} whatever its memory holds.  -1 (no children) stays -1; a first_child is below
// 2^24 in every tree of these forms (the host runs a plan whose capacity reaches 2^24 by the count-1 rule).  A node of count 1
// has mask 0: the count-1 rule is the special case.  The host marks the trees (TreeMeta::virgin holds the mode) and every reader
// goes by it: the kernel's own selection and plan read-out, uct_reroot_kernel, uct_path_count_kernel and the export (below).
// Re-rooted trees are whole and their words plain.
#pragma once

namespace mp {

enum UctTreeMode { kUctTreeWhole = 0, kUctTreeCount1 = 1, kUctTreeMasked = 2 };

constexpr int kUctMaskShift = 24;
constexpr int kUctChildBits = (1 << kUctMaskShift) - 1;

// the first child's id and the visited mask of a masked tree's first_child word
constexpr int uct_word_child(int w) { return w < 0 ? -1 : w & kUctChildBits; }
constexpr unsigned uct_word_mask(int w) { return w < 0 ? 0u : (unsigned)w >> kUctMaskShift; }
constexpr bool uct_word_stored(int w, int a) { return ((uct_word_mask(w) >> a) & 1u) != 0u; }

// The instantiations of uct_kernel<AT, ENV, SP, MK, IL, QD> that take part: the one-lane LDS-resident form (ENV 3) and the gather
// forms (ENV 0 / 4) for |A| <= 5, in the group-interleaved layout; none of them gains a register spill or loses a wave per SIMD.
// The LDS-resident form of |A| = 6 would spill two VGPRs (12 bytes of scratch) and is left out.  Listed policies (MK) hold phantom
// counts in their groups; CartPole, per-state policies and the four-lane form keep their complete trees and were not tried
// (profiles/uct_virgin_groups.md).
constexpr bool uct_virgin_form(int AT, int ENV, bool SP, bool MK, int IL, bool QD)
{
    return IL == 2 && !SP && !MK && !QD && AT >= 2 && AT <= 5 && (ENV == 3 || ENV == 0 || ENV == 4);
}

// The instantiations that keep the visited mask: those of uct_virgin_form (profiles/uct_visited_mask.md has their registers).
constexpr bool uct_mask_form(int AT, int ENV, bool SP, bool MK, int IL, bool QD)
{
    return uct_virgin_form(AT, ENV, SP, MK, IL, QD);
}

// The export's reading of a tree that may hold unstored nodes: nodes h[0 .. tcap) in id order as copied from the device.  Makes
// the tree whole -- the constant node wherever the mode's rule says a child was never stored, the first_child words plain -- and
// returns the number of node slots in use (the closure of the first_child links, as the export computes it).  Ids grow from
// parent to child, so one forward pass sees a parent before its group.  kUctTreeWhole: the closure alone.
template <typename Node>
inline int uct_virgin_fill(Node *h, int tcap, int A, int mode)
{
    int n = 1;
    for (int i = 0; i < n && i < tcap; ++i) {
        const int w = h[i].first_child;
        if (w < 0) continue;
        const int fc = mode == kUctTreeMasked ? uct_word_child(w) : w;
        h[i].first_child = fc;
        for (int a = 0; a < A && fc + a < tcap; ++a) {
            const bool unstored = mode == kUctTreeMasked ? !uct_word_stored(w, a) : (mode == kUctTreeCount1 && h[i].count == 1);
            if (unstored) { h[fc + a].value = 0.0; h[fc + a].count = 0; h[fc + a].first_child = -1; }
        }
        if (fc + A > n) n = fc + A;
    }
    return n;
}

} // namespace mp
