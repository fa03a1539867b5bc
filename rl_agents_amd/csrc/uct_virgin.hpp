// uct_virgin.hpp -- the rule that lets uct_kernel leave the zero groups of its expansions out of memory, for everything that
// reads its trees.  Plain C++ (no HIP): the kernel, the host readers of uct.hip and a stand-alone host test include it.
//
// A UCT node expands on its FIRST visit only (mcts.py:151-154: the selection stops at a node without children, which then
// expands), and a later visit descends into one of the children and backs it up.  So in a tree without phantom slots
//     count == 1 and first_child >= 0   =>   the |A| children are all {value 0.0, count 0, first_child -1}
// (re-rooted trees included: a node that expands late there has count >= 2).  A fresh-tree plan of a form that takes part
// (uct_virgin_form) with the default tree stores writes no such group: its memory holds whatever was there until the first entry
// completes it.  The host marks such trees (TreeMeta::virgin) and every reader substitutes the constant node below a count-1
// node: the kernel's own selection and plan read-out, uct_reroot_kernel, uct_path_count_kernel and the export (below).
#pragma once

namespace mp {

// The instantiations of uct_kernel<AT, ENV, SP, MK, IL, QD> that take part: the one-lane LDS-resident form (ENV 3) and the gather
// forms (ENV 0 / 4) for |A| <= 5, in the group-interleaved layout; none of them gains a register spill or loses a wave per SIMD.
// The LDS-resident form of |A| = 6 would spill two VGPRs (12 bytes of scratch) and is left out.  Listed policies (MK) hold phantom
// counts in their groups; CartPole, per-state policies and the four-lane form keep their complete trees and were not tried
// (profiles/uct_virgin_groups.md).
constexpr bool uct_virgin_form(int AT, int ENV, bool SP, bool MK, int IL, bool QD)
{
    return IL == 2 && !SP && !MK && !QD && AT >= 2 && AT <= 5 && (ENV == 3 || ENV == 0 || ENV == 4);
}

// The export's reading of a tree that may hold unstored groups: nodes h[0 .. tcap) in id order as copied from the device.  Fills
// the children of every count-1 node with the constant node and returns the number of node slots in use (the closure of the
// first_child links, as the export computes it).  Ids grow from parent to child, so one forward pass sees a parent before its
// group.  `virgin` false: the closure alone.
template <typename Node>
inline int uct_virgin_fill(Node *h, int tcap, int A, bool virgin)
{
    int n = 1;
    for (int i = 0; i < n && i < tcap; ++i) {
        const int fc = h[i].first_child;
        if (fc < 0) continue;
        if (virgin && h[i].count == 1)
            for (int a = 0; a < A && fc + a < tcap; ++a) { h[fc + a].value = 0.0; h[fc + a].count = 0; h[fc + a].first_child = -1; }
        if (fc + A > n) n = fc + A;
    }
    return n;
}

} // namespace mp
