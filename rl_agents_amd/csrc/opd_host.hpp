// opd_host.hpp -- the host side that mp_opd_plan (opd.hip) and mp_ropd_plan (ropd.hip) share: the shape of a call and the
// choice of kernel form, the gamma-power tables, the staging of the outputs, and the skeleton of a tree export.  Each entry
// point keeps its own argument checks and messages, its own node arrays and its own kernels.
#pragma once
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "common.hpp"
#include "opd_closing.hpp"

namespace mp {

// ---- sizes and kernel form of one plan call.  Three forms (opd.hip: opd_kernel<EXPG>, opd_wide_kernel):
//   !glb && !expg   upper-bound array AND parent map in LDS (lds_full): lowest latency per root
//   !glb && expg    the parent map in HBM (lds_bounds): one more root per CU at budget 5000
//   glb             the bounds array in HBM/L2, LDS only holds the window of the closing lower-bound pass (lds_win)
// LDS-resident while every root of the batch fits on the chip that way.  Test hooks, read at every call:
//   MP_OPD_MODEL=lds|ldsx|global   the form (ldsx = expg)            MP_OPD_WIDE=cls      residue-class layout of the wide form
//   MP_OPD_CLOSING=chain           the node-array closing even where closing_compact fits
//   MP_OPD_LOOP=0                  the general main loops
struct OpdShape {
    int K;   // expansions: budget // |A| (deterministic.py:118)
    int cap; // node slots per root, 1 + K |A|
    int T;   // row length of a residue class in the bounds array: odd, >= ceil(cap / 64)
    int Tsib, lgP; // sibling layout of the wide form (default): groups of |A| slots, ceil((K + 1) / 64) groups per row, one cache
                   // line of padding so that rows do not all start in the same channels; a leaf's code is (group << lgP) | child
    int chunk;     // wide form: expansions per LDS window of the closing pass (power of two <= 64, window <= 4 KB)
    size_t lds_full, lds_bounds, lds_win;
    bool glb, expg, sib;
    bool nonneg; // every finite bound is >= +0.0 (rewards are range-checked, gamma in [0, 1), terminal reward >= 0): the cheaper
                 // cross-lane maxima (wave.hpp) and the batched-load loops of ropd.hip
    bool closing_chain;
    size_t lds() const { return glb ? lds_win : (expg ? lds_bounds : lds_full); }
    size_t kslots() const { return (size_t)(K > 0 ? K : 1); } // row length of the parent map
};

inline OpdShape opd_shape(const mp_ctx *ctx, int A, int budget, int n_roots, double gamma, double terminal_reward)
{
    OpdShape s;
    s.K = budget / A;
    const long cap = 1 + (long)s.K * A;
    s.cap = (int)cap;
    s.T = (int)((cap + 63) / 64) | 1;
    s.lgP = 0;
    while ((1 << s.lgP) < A) ++s.lgP;
    s.Tsib = ((s.K + 1 + 63) / 64) * A + 16;
    s.chunk = 64;
    while (s.chunk > 1 && (size_t)s.chunk * A * sizeof(double) > 4096) s.chunk >>= 1;
    s.lds_bounds = (size_t)64 * s.T * sizeof(double); // (T >= 1: never zero)
    s.lds_full = s.lds_bounds + s.kslots() * sizeof(int32_t);
    s.lds_win = (size_t)s.chunk * A * sizeof(double);
    const size_t avail = kLdsBytes - 1024;
    const long cus = ctx->prop.multiProcessorCount;
    const char *force = getenv("MP_OPD_MODEL");
    s.glb = s.lds_bounds > avail || n_roots > cus * (long)(avail / s.lds_bounds);
    if (force && force[0] == 'g') s.glb = true;
    if (force && force[0] == 'l' && s.lds_bounds <= avail) s.glb = false;
    // bounds in LDS: keep the parent map there too while that costs no residency
    s.expg = !s.glb && (s.lds_full > avail || n_roots > cus * (long)(avail / s.lds_full));
    if (force && !s.glb && force[1] == 'd' && force[2] == 's' && force[3] == 'x') s.expg = true;
    const char *wide = getenv("MP_OPD_WIDE"), *closing = getenv("MP_OPD_CLOSING"), *loop = getenv("MP_OPD_LOOP");
    s.sib = !(wide && wide[0] == 'c');
    s.closing_chain = closing && closing[0] == 'c';
    s.nonneg = gamma >= 0 && gamma < 1 && terminal_reward >= 0 && !(loop && loop[0] == '0');
    return s;
}

// the LDS-resident kernels (opd_kernel, ropd_kernel) close on the node array when told to, or when the tables of
// opd_closing.hpp do not fit the bounds array they reuse: the kernels' own test, asked from the host for the form's name
inline bool opd_closing_on_nodes(const OpdShape &s, int A)
{
    return s.closing_chain || !closing_compact_fits(s.K, A, s.cap, 64L * s.T * 8);
}

// ---- gamma-power tables for depths <= K + 1, host libm (bit-equal to Python's float **):
// g1[d] = gamma ** (d - 1) (d >= 1), gdiv[d] = gamma ** d / (1 - gamma), tdiv[d] = terminal_reward * gamma ** d / (1 - gamma)
inline int opd_gamma_tables(mp_ctx *ctx, int K, double gamma, double terminal_reward, const double **g1, const double **gdiv,
                            const double **tdiv)
{
    const int D = K + 2;
    std::vector<double> tab((size_t)3 * D);
    for (int d = 0; d < D; ++d) {
        tab[d] = d >= 1 ? pow(gamma, (double)(d - 1)) : 0.0;
        tab[D + d] = pow(gamma, (double)d) / (1 - gamma);
        tab[2 * D + d] = terminal_reward * pow(gamma, (double)d) / (1 - gamma);
    }
    double *d_tab = nullptr;
    MP_TRY(upload_tables(ctx, 2, tab, &d_tab));
    *g1 = d_tab; *gdiv = d_tab + D; *tdiv = d_tab + 2 * D;
    return MP_OK;
}

// ---- the caller's arrays of a plan call (each may be null except rng_state) and their device side: the generator records in,
// the parent map + node counts (kept on the ctx for the tree export) and the six result arrays out
struct OpdResults {
    uint64_t *rng_state;
    int32_t *plans, *plan_len;
    double *root_lower, *root_upper;
    int64_t *env_steps;
    int32_t *status;
};

inline int opd_stage(mp_ctx *ctx, const OpdShape &s, int n_roots, int max_plan_len, int mem, int rmem, const OpdResults &r,
                     uint64_t **rng, OpdOut *o)
{
    const size_t n = (size_t)n_roots;
    MP_TRY(ws_get(ctx, WS_TREE7, n * s.kslots() + n, &o->expanded));
    o->n_nodes_out = o->expanded + n * s.kslots();
    MP_TRY(stage_in(ctx, WS_IO2, (const uint64_t *)r.rng_state, n * 6, rmem, rng));
    MP_TRY(stage_out_alloc(ctx, WS_IO3, r.plans, n * max_plan_len, mem, &o->plans));
    MP_TRY(stage_out_alloc(ctx, WS_IO4, r.plan_len, n, mem, &o->plan_len));
    MP_TRY(stage_out_alloc(ctx, WS_IO5, r.root_lower, n, mem, &o->root_lower));
    MP_TRY(stage_out_alloc(ctx, WS_IO6, r.root_upper, n, mem, &o->root_upper));
    MP_TRY(stage_out_alloc(ctx, WS_IO7, r.status, n, mem, &o->status));
    MP_TRY(stage_out_alloc(ctx, WS_IO8, r.env_steps, n, mem, &o->env_steps));
    return MP_OK;
}

inline int opd_unstage(mp_ctx *ctx, int n_roots, int max_plan_len, int mem, int rmem, const OpdResults &r, const uint64_t *rng,
                       const OpdOut &o)
{
    const size_t n = (size_t)n_roots;
    MP_TRY(stage_out_copy(ctx, r.rng_state, rng, n * 6, rmem));
    MP_TRY(stage_out_copy(ctx, r.plans, o.plans, n * max_plan_len, mem));
    MP_TRY(stage_out_copy(ctx, r.plan_len, o.plan_len, n, mem));
    MP_TRY(stage_out_copy(ctx, r.root_lower, o.root_lower, n, mem));
    MP_TRY(stage_out_copy(ctx, r.root_upper, o.root_upper, n, mem));
    MP_TRY(stage_out_copy(ctx, r.status, o.status, n, mem));
    MP_TRY(stage_out_copy(ctx, r.env_steps, o.env_steps, n, mem));
    if (mem == MP_MEM_HOST) MP_HIP(hipStreamSynchronize(ctx->stream));
    return MP_OK;
}

// ---- tree export.  The tree of the last plan call stays in the workspace of the ctx: per-root node arrays of ctx->tree.cap
// slots each (opd_pull reads the first n slots of one), the parent map and the node counts in WS_TREE7.
inline int opd_pull(mp_ctx *ctx, int slot, int root, int n, size_t elt, void *dst)
{
    MP_HIP(hipMemcpy(dst, (const char *)ctx->ws[slot].p + (size_t)root * ctx->tree.cap * elt, (size_t)n * elt, hipMemcpyDeviceToHost));
    return MP_OK;
}

// the number of node slots root `root` used and its parent map (exp[k] = the node expansion k expanded, -1: not taken)
inline int opd_pull_expanded(mp_ctx *ctx, int root, int32_t *n, std::vector<int32_t> &exp)
{
    const size_t kk = (size_t)(ctx->tree.K > 0 ? ctx->tree.K : 1);
    MP_HIP(hipSetDevice(ctx->device));
    MP_HIP(hipStreamSynchronize(ctx->stream));
    const int32_t *d_exp = (const int32_t *)ctx->ws[WS_TREE7].p;
    MP_HIP(hipMemcpy(n, d_exp + (size_t)ctx->tree.n_roots * kk + root, sizeof(int32_t), hipMemcpyDeviceToHost));
    exp.resize(kk);
    MP_HIP(hipMemcpy(exp.data(), d_exp + (size_t)root * kk, kk * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MP_OK;
}

// What both exports derive from the parent map.  The k-th expansion created the node slots 1 + kA .. 1 + kA + A - 1 under
// exp[k]; the slot of an unavailable action (deterministic.py:32-35) is a PHANTOM, not a node of the tree: dropped, the
// others renumbered in order.
struct OpdSkeleton {
    std::vector<int32_t> fc, par, id; // per slot: first child slot (-1: a leaf), parent slot, exported index (-1: phantom)
    std::vector<int64_t> sz;          // kept slots in the subtree, the slot itself included
    int kept = 0;

    // the links of slot i (kept), written at its exported index; any array may be null
    void links(int i, int A, int32_t *parent, int32_t *action, int64_t *count, int32_t *first_child, int32_t *n_children) const
    {
        const int o = id[i];
        if (parent) parent[o] = i == 0 ? -1 : id[par[i]];
        if (action) action[o] = i == 0 ? -1 : (i - 1) % A;
        // deterministic.py:62-63: every node on the root..child sequence gets +1 per created child;
        // count = 1 (initial) + size of own subtree for non-root nodes, root: 1 + #descendants
        if (count) count[o] = i == 0 ? sz[0] : 1 + sz[i];
        int first = -1, nc = 0;
        if (fc[i] >= 0)
            for (int a = 0; a < A; ++a) {
                const int c = id[fc[i] + a];
                if (c < 0) continue;
                if (first < 0) first = c;
                ++nc;
            }
        if (first_child) first_child[o] = first;
        if (n_children) n_children[o] = nc;
    }
};

// upper[]: the kernels store leaf upper bounds only (-inf marks an expanded node); an expanded node's is filled in here as
// the max over its children, bottom-up in reverse creation order (children have larger ids than their parent).
template <class IsPhantom>
inline OpdSkeleton opd_skeleton(const std::vector<int32_t> &exp, int n, int A, int K, IsPhantom is_phantom, double *upper)
{
    OpdSkeleton t;
    t.fc.assign((size_t)n, -1); t.par.assign((size_t)n, -1); t.id.assign((size_t)n, -1); t.sz.assign((size_t)n, 0);
    for (int k = 0; k < K && 1 + (k + 1) * A <= n; ++k)
        if (exp[k] >= 0 && exp[k] < n) t.fc[exp[k]] = 1 + k * A;
    for (int i = 1; i < n; ++i) t.par[i] = exp[(i - 1) / A];
    for (int i = n - 1; i >= 0; --i)
        if (t.fc[i] >= 0) {
            double m = upper[t.fc[i]];
            for (int a = 1; a < A; ++a)
                if (upper[t.fc[i] + a] > m) m = upper[t.fc[i] + a];
            upper[i] = m;
        }
    for (int i = 0; i < n; ++i)
        if (!is_phantom(i)) t.id[i] = t.kept++;
    for (int i = n - 1; i >= 0; --i) {
        if (t.id[i] < 0) continue;
        t.sz[i] += 1;
        if (i > 0) t.sz[t.par[i]] += t.sz[i];
    }
    return t;
}

} // namespace mp
