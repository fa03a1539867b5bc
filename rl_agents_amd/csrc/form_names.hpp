// form_names.hpp -- the names mp_last_kernel_variant reports, one small function per planner.  An entry point passes the
// selectors it launched with, after every override and fallback, to its function; mp_kernel_form_names (api.hip) loops the
// same functions over their selector ranges.  Host only.  A name fits mp_ctx::last_variant (kFormNameBytes with the NUL).
#pragma once
#include <stdio.h>
#include <string.h>

#include <string>

namespace mp {

constexpr int kFormNameBytes = 48;

struct FormName {
    char s[kFormNameBytes];
    const char *c_str() const { return s; }
};

inline void form_record(char (&dst)[kFormNameBytes], const FormName &n) { snprintf(dst, sizeof(dst), "%s", n.s); }

// ---- UCT (uct.hip: the index is its UctForm), batched VI (vi.hip), OLOP, BRUE, GBOP-D
constexpr int kUctForms = 11;
inline FormName uct_form_name(int form)
{
    static const char *const name[kUctForms] = {"global", "global_spill", "ldsr", "quad", "lone", "lone_mw", "lone_each", "row_each",
                                                "row_shared", "cartpole", "policy"};
    FormName n;
    snprintf(n.s, sizeof(n.s), "uct_%s", name[form]);
    return n;
}
// (the same name in static storage: mp_uct_choose_form hands out a pointer)
inline const char *uct_form_name_static(int form)
{
    static const struct Names {
        FormName n[kUctForms];
        Names() { for (int f = 0; f < kUctForms; ++f) n[f] = uct_form_name(f); }
    } names;
    return names.n[form].s;
}

// the register forms of the batched VI: states per thread, threads per workgroup
constexpr int kViBatchRegForms = 7;
constexpr int kViBatchReg[kViBatchRegForms][2] = {{1, 64}, {2, 64}, {2, 128}, {2, 256}, {4, 256}, {4, 512}, {4, 1024}};
// (entry i is instantiated for the compile-time |A| `at`: four states of 1024 threads hold the rows of at most four actions)
constexpr bool vi_batch_reg_exists(int at, int i) { return at > 0 && (kViBatchReg[i][1] < 1024 || at <= 4); }
inline FormName vi_batch_reg_name(int own, int block)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "vi_batch_reg<%d,%d>", own, block);
    return n;
}
inline FormName vi_batch_cluster_name(int k) // 2, 4 or 8 workgroups per MDP
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "vi_batch_cluster%d", k);
    return n;
}
enum ViBatchWg { VB_WG_STREAM, VB_WG_LDS, VB_WG_GLOBAL, VB_WG_COUNT };
inline FormName vi_batch_wg_name(int kind)
{
    static const char *const name[VB_WG_COUNT] = {"stream", "lds", "global"};
    FormName n;
    snprintf(n.s, sizeof(n.s), "vi_batch_wg_%s", name[kind]);
    return n;
}
// (one of the 13 names above in static storage: mp_vi_batch_geometry hands out a pointer)
inline const char *vi_batch_form_name_static(const FormName &n)
{
    static const struct Names {
        FormName n[kViBatchRegForms + 3 + VB_WG_COUNT];
        Names()
        {
            int i = 0;
            for (const auto &f : kViBatchReg) n[i++] = vi_batch_reg_name(f[0], f[1]);
            for (int k = 2; k <= 8; k *= 2) n[i++] = vi_batch_cluster_name(k);
            for (int k = 0; k < VB_WG_COUNT; ++k) n[i++] = vi_batch_wg_name(k);
        }
    } names;
    for (const FormName &s : names.n)
        if (!strcmp(s.s, n.s)) return s.s;
    return "";
}

inline FormName slots_form_name(const char *planner, bool keep) // OLOP, BRUE: the trees kept for export, or slots shared by waves
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "%s_global%s", planner, keep ? "" : "_slots");
    return n;
}
inline FormName olop_form_name(bool keep) { return slots_form_name("olop", keep); }
inline FormName brue_form_name(bool keep) { return slots_form_name("brue", keep); }
// OLOP on a stochastic finite MDP (mp_olop_plan_stochastic, olop.hip): named by the model's rows.  Listed by
// mp_olop_stoch_form_names -- NOT by all_form_names below, as for Sparse Sampling.
inline FormName olop_stoch_form_name(bool sparse)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "olop_stoch_%s", sparse ? "sparse" : "dense");
    return n;
}
inline FormName gbopd_form_name(bool use_lds)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "gbopd_wave_%s", use_lds ? "lds" : "global");
    return n;
}
// GBOP (gbop.hip): named by the model's rows (its MP_MODE_* of mi355plan.h, which common.hpp includes before this header) and
// the placement of the bounds.  Listed by mp_gbop_form_names -- NOT by all_form_names below, as for Sparse Sampling.
inline FormName gbop_form_name(int mode, bool use_lds)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "gbop_%s_%s", mode == MP_MODE_DETERMINISTIC ? "table" : mode == MP_MODE_SPARSE ? "sparse" : "dense",
             use_lds ? "lds" : "global");
    return n;
}
inline std::string gbop_form_names()
{
    std::string out;
    for (int mode : {MP_MODE_DETERMINISTIC, MP_MODE_STOCHASTIC, MP_MODE_SPARSE})
        for (int l = 1; l >= 0; --l) { out += gbop_form_name(mode, l != 0).s; out += '\n'; }
    out.pop_back();
    return out;
}

// Sparse Sampling (sparse_sampling.hip): the frames in LDS or in a global workspace.  Reported by mp_last_kernel_variant after a
// call and listed by the planner's own mp_ss_form_names -- NOT by all_form_names below, whose list is pinned name for name
// by a table of the planners it covers.
inline FormName ss_form_name(bool use_lds)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "ss_wave_%s", use_lds ? "lds" : "global");
    return n;
}

// OLOP and BRUE on a batch model with one MDP per root (mp_olop_plan_models / mp_brue_plan_models, each_host.hpp): the root's
// table in LDS or read from global memory, with the `_slots` suffix of slots_form_name.  planner: 0 = OLOP, 1 = BRUE.  Listed by
// mp_each_form_names -- NOT by all_form_names below, as for Sparse Sampling.
inline FormName each_form_name(int planner, bool lds, bool keep)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "%s_each_%s%s", planner == 0 ? "olop" : "brue", lds ? "lds" : "global", keep ? "" : "_slots");
    return n;
}
inline std::string each_form_names()
{
    std::string out;
    for (int planner = 0; planner < 2; ++planner)
        for (int lds = 1; lds >= 0; --lds)
            for (int keep = 1; keep >= 0; --keep) { out += each_form_name(planner, lds != 0, keep != 0).s; out += '\n'; }
    return out;
}

// Sparse Sampling on a batch model with one MDP per root (mp_ss_plan_models, each_host.hpp): the root's table in LDS or read from
// global memory (the trees have no `_slots` form: every root's is kept, or root 0's alone).  Listed by mp_ss_each_form_names --
// mp_each_form_names and mp_ss_form_names are pinned name for name by the tests of the planners they cover.
inline FormName ss_each_form_name(bool lds)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "ss_each_%s", lds ? "lds" : "global");
    return n;
}
inline std::string ss_each_form_names() { return std::string(ss_each_form_name(true).s) + "\n" + ss_each_form_name(false).s + "\n"; }

// ---- single-model value iteration (vi.hip: mp_vi_solve, mp_vi_solve_v, mp_vi_solve_v_robust, mp_vi_sweeps, mp_vi_backup):
// the form of the launch that produced the returned values.  Reported by mp_last_kernel_variant after a call and listed by
// mp_vi_form_names -- NOT by all_form_names below, as for Sparse Sampling.
// Deterministic tables: one workgroup with everything in LDS (VD_SMALL), one persistent grid (VD_PERSIST: `at` x `models` is
// one of kViPersistForms) or a launch per sweep (VD_CHAIN; graph: replayed from the captured graph).  at: the unrolled |A|,
// 0 = the loop form.
enum ViDetKind { VD_SMALL, VD_PERSIST, VD_CHAIN };
struct ViDetForm {
    int kind, at, models;
    bool graph;
};
constexpr int kViDetUnrolled[6] = {2, 3, 4, 5, 6, 8};
inline int vi_det_unrolled(int A)
{
    for (int a : kViDetUnrolled)
        if (a == A) return A;
    return 0;
}
constexpr int kViPersistForms = 19;
constexpr int kViPersist[kViPersistForms][2] = {{2, 1}, {3, 1}, {4, 1}, {5, 1}, {6, 1}, {8, 1}, {2, 2}, {3, 2}, {4, 2}, {5, 2},
                                                {6, 2}, {8, 2}, {2, 3}, {3, 3}, {4, 3}, {5, 3}, {2, 4}, {3, 4}, {4, 4}};
inline bool vi_persist_form_exists(int A, int M)
{
    for (const auto &f : kViPersist)
        if (f[0] == A && f[1] == M) return true;
    return false;
}
inline FormName vi_det_form_name(const ViDetForm &f)
{
    FormName n;
    char a[8];
    if (f.at) snprintf(a, sizeof(a), "%d", f.at);
    else snprintf(a, sizeof(a), "any");
    if (f.kind == VD_SMALL) snprintf(n.s, sizeof(n.s), "vi_det_small_a%s", a);
    else if (f.kind == VD_PERSIST) snprintf(n.s, sizeof(n.s), "vi_det_persist_a%s_m%d", a, f.models);
    else snprintf(n.s, sizeof(n.s), "vi_det_chain_a%s%s", a, f.graph ? "_graph" : "");
    return n;
}
inline FormName vi_sparse_form_name(bool big) // more than 128 next states per (s, a): the pairwise recursion
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "vi_sparse%s", big ? "_big" : "");
    return n;
}
// Dense rows: numpy's order (exact: nbt = the unrolled 8-element steps of a leaf, place = where the lanes read V from, in the
// order of vi.hip's VI_V_* values) or the matrix cores (split: the columns cut into segments).
constexpr int kViExactNbt[5] = {8, 10, 12, 14, 16};
inline int vi_exact_nbt(int nb)
{
    for (int t : kViExactNbt)
        if (nb <= t) return t;
    return kViExactNbt[4];
}
struct ViDenseForm {
    bool exact;
    int nbt, place;
    bool split;
};
inline FormName vi_dense_form_name(const ViDenseForm &f)
{
    static const char *const place[3] = {"global", "lds", "pieces"};
    FormName n;
    if (f.exact) snprintf(n.s, sizeof(n.s), "vi_dense_exact_n%d_%s", f.nbt, place[f.place]);
    else snprintf(n.s, sizeof(n.s), "vi_dense_mfma%s", f.split ? "_split" : "");
    return n;
}
inline std::string vi_form_names()
{
    std::string out;
    auto add = [&](const FormName &n) { out += n.s; out += '\n'; };
    for (int kind = VD_SMALL; kind <= VD_CHAIN; kind += 2)
        for (int graph = 0; graph <= (kind == VD_CHAIN ? 1 : 0); ++graph) {
            for (int a : kViDetUnrolled) add(vi_det_form_name({kind, a, 1, graph != 0}));
            add(vi_det_form_name({kind, 0, 1, graph != 0}));
        }
    for (const auto &f : kViPersist) add(vi_det_form_name({VD_PERSIST, f[0], f[1], false}));
    add(vi_sparse_form_name(false));
    add(vi_sparse_form_name(true));
    for (int t : kViExactNbt)
        for (int place = 1; place <= 3; ++place) add(vi_dense_form_name({true, t, place % 3, false}));
    add(vi_dense_form_name({false, 0, 0, false}));
    add(vi_dense_form_name({false, 0, 0, true}));
    return out;
}

// ---- OPD (opd.hip) and robust OPD (ropd.hip).  any_a: |A| > 64, the plain kernel.  Else glb: the wide kernel in its sibling
// (sib) or residue-class layout; !glb: the LDS-resident kernel, the parent map in HBM with expg, the closing pass on the node
// array with chain.  nonneg picks the cheaper main loops everywhere.
// OPD only: small = the wide kernel's two-slots-per-lane re-scan.  Robust OPD only: mb = the batched-load main loop of the
// LDS-resident kernel (0 the generic one, 1 up to two models, 2 up to four).
struct OpdForm {
    bool any_a, glb, expg, sib, small, nonneg, chain;
    int mb;
};
inline FormName opd_form_name(const OpdForm &f)
{
    FormName n;
    if (f.any_a) snprintf(n.s, sizeof(n.s), "opd_any");
    else if (f.glb) snprintf(n.s, sizeof(n.s), "opd_wide_%s%s%s", f.sib ? "sib" : "cls", f.small ? "_small" : "", f.nonneg ? "" : "_gen");
    else snprintf(n.s, sizeof(n.s), "opd_%s%s%s", f.expg ? "ldsx" : "lds", f.nonneg ? "" : "_gen", f.chain ? "_chain" : "");
    return n;
}
inline FormName ropd_form_name(const OpdForm &f)
{
    FormName n;
    if (f.any_a) snprintf(n.s, sizeof(n.s), "ropd_any");
    else if (f.glb) snprintf(n.s, sizeof(n.s), "ropd_wide_%s%s", f.sib ? "sib" : "cls", f.nonneg ? "" : "_gen");
    else snprintf(n.s, sizeof(n.s), "ropd_%s%s%s", f.expg ? "ldsx" : "lds", f.mb == 1 ? "_m2" : f.mb == 2 ? "_m4" : "_gen", f.chain ? "_chain" : "");
    return n;
}

// ---- state-aware OPD (saopd.hip): the kernel of the LAST launch of the call.  One planner per lane, or per wavefront with
// everything in global memory, with the dictionaries in LDS (dict) or with the arena in LDS too (lds); ordered: the dispatch
// order was sorted (saopd_order_kernel ran); retry: the call rolled back and ran again.
struct SaopdForm {
    bool wave, dict, lds, ordered, retry;
};
// (the lane kernel takes no dispatch order; a retry of the all-in-LDS form runs on another form)
inline bool saopd_form_possible(const SaopdForm &f)
{
    return !(f.lds && f.dict) && (f.wave || !(f.dict || f.lds || f.ordered)) && !(f.lds && f.retry);
}
inline FormName saopd_form_name(const SaopdForm &f)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "saopd_%s%s%s", !f.wave ? "lane" : f.lds ? "wave_lds" : f.dict ? "wave_dict" : "wave", f.ordered ? "_ordered" : "",
             f.retry ? "_retry" : "");
    return n;
}
// (the same name in static storage: mp_saopd_choose_form hands out pointers)
inline const char *saopd_form_name_static(const SaopdForm &f)
{
    static const struct Names {
        FormName n[16];
        Names() { for (int i = 0; i < 16; ++i) n[i] = saopd_form_name({(i & 12) != 0, (i & 12) == 8, (i & 12) == 12, (i & 2) != 0, (i & 1) != 0}); }
    } names;
    return names.n[(!f.wave ? 0 : f.lds ? 12 : f.dict ? 8 : 4) | (f.ordered ? 2 : 0) | (f.retry ? 1 : 0)].s;
}

// ---- UCT on stochastic models (uct_stoch.hip).  wbk: the form the step records really have (0 rows + thresholds, 2 / 4 fused
// records of that many successors, 1 the compact 16-byte records); p16: 16-bit path entries; at: the unrolled |A| in 2..8 or
// 0, the loop form; pol: per-state policies (32-bit path entries only)
inline bool uct_stoch_form_possible(int wbk, bool p16, int at, bool pol)
{
    return (wbk == 0 || wbk == 1 || wbk == 2 || wbk == 4) && (at == 0 || (at >= 2 && at <= 8)) && !(pol && p16);
}
inline FormName uct_stoch_form_name(int wbk, bool p16, int at, bool pol)
{
    FormName n;
    char a[8];
    if (at) snprintf(a, sizeof(a), "%d", at);
    else snprintf(a, sizeof(a), "any");
    snprintf(n.s, sizeof(n.s), "uct_stoch_r%d_p%d_a%s%s", wbk, p16 ? 16 : 32, a, pol ? "_policy" : "");
    return n;
}

// every name an entry point can record, one per line (Sparse Sampling's two are listed by mp_ss_form_names, single-model
// value iteration's by mp_vi_form_names, the one-MDP-per-root forms of OLOP and BRUE by mp_each_form_names)
inline std::string all_form_names()
{
    std::string out;
    auto add = [&](const FormName &n) { out += n.s; out += '\n'; };
    for (int f = 0; f < kUctForms; ++f) add(uct_form_name(f));
    for (int i = 0; i < kViBatchRegForms; ++i) add(vi_batch_reg_name(kViBatchReg[i][0], kViBatchReg[i][1]));
    for (int k = 2; k <= 8; k *= 2) add(vi_batch_cluster_name(k));
    for (int k = 0; k < VB_WG_COUNT; ++k) add(vi_batch_wg_name(k));
    for (int keep = 1; keep >= 0; --keep) { add(olop_form_name(keep)); add(brue_form_name(keep)); }
    for (int l = 1; l >= 0; --l) add(gbopd_form_name(l));
    for (int robust = 0; robust < 2; ++robust) {
        OpdForm f = {};
        f.any_a = true;
        add(robust ? ropd_form_name(f) : opd_form_name(f));
        f.any_a = false;
        for (int expg = 0; expg < 2; ++expg)
            for (int v = 0; v < (robust ? 3 : 2); ++v)
                for (int chain = 0; chain < 2; ++chain) {
                    f.glb = false; f.expg = expg; f.chain = chain;
                    f.nonneg = robust ? v != 0 : v == 0; f.mb = robust ? v : 0;
                    add(robust ? ropd_form_name(f) : opd_form_name(f));
                }
        for (int sib = 1; sib >= 0; --sib)
            for (int small = robust ? 0 : 1; small >= 0; --small)
                for (int nonneg = 1; nonneg >= 0; --nonneg) {
                    f.glb = true; f.sib = sib; f.small = small; f.nonneg = nonneg;
                    add(robust ? ropd_form_name(f) : opd_form_name(f));
                }
    }
    for (int kind = 0; kind < 4; ++kind)
        for (int ordered = 0; ordered < 2; ++ordered)
            for (int retry = 0; retry < 2; ++retry) {
                const SaopdForm f = {kind != 0, kind == 2, kind == 3, ordered != 0, retry != 0};
                if (saopd_form_possible(f)) add(saopd_form_name(f));
            }
    static const int wbks[4] = {0, 2, 4, 1};
    for (int pol = 0; pol < 2; ++pol)
        for (int w = 0; w < 4; ++w)
            for (int p16 = 1; p16 >= 0; --p16)
                for (int at = 0; at <= 8; ++at)
                    if (at != 1 && uct_stoch_form_possible(wbks[w], p16, at, pol)) add(uct_stoch_form_name(wbks[w], p16, at, pol));
    return out;
}

} // namespace mp
