// uct_host.hpp -- the host side that mp_uct_plan* (uct.hip) and mp_uct_plan_stochastic* (uct_stoch.hip) share: the arguments of
// a plan call, the small per-call tables, the bookkeeping of kept subtrees and the skeleton of a re-rooting.  The caller's arrays
// are named in a WaveIo (wave_host.hpp).  Each entry point keeps its own argument checks and messages, its TE rule and table kind,
// its args struct, its tree buffers, its way of staging (uct.hip: zero-copy for the whole call or chunk copies; uct_stoch.hip:
// per array, wave_stage) and its kernels.
#pragma once
#include <math.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "wave_host.hpp"

namespace mp {

// ---- what the extern "C" wrappers hand to uct_plan_impl / uct_stoch_plan_impl, in the order of the C ABI.  pol: a per-state
// policy (then prior_p / rollout_p are NULL); closed_loop and env_rng_state: the stochastic entry points only.
struct UctPlan {
    mp_model *model;
    const mp_policy *pol;
    int32_t n_roots;
    const void *root_state;
    const int32_t *root_steps;
    int32_t episodes, horizon;
    double gamma, temperature;
    const double *prior_p, *rollout_p;
    int32_t closed_loop;
    uint64_t *rng_state;
    const uint64_t *env_rng_state;
    int32_t max_plan_len;
    int32_t *plans, *plan_len;
    double *root_value;
    int64_t *root_child_count;
    double *root_child_value;
    int64_t *env_steps;
    int32_t mem;
};

// ---- the small per-call tables [gpow (H + 1) | cdf thresholds (A) | tpv (A) | rcp (TE + 1) | tpdiv (A)(TE + 2)], computed on
// the host exactly as Python computes them; TE: the largest visit count the quotient tables hold (they live in LDS: counts
// beyond take the IEEE division in the kernel -- the same quotients).  prior_p / rollout_p NULL: a per-state policy plans
// (priors 0, a uniform rollout row).
struct UctTables { size_t cdf, tpv, rcp, tpdiv, n; }; // offsets in doubles, and the length

inline UctTables uct_tables(int H, int A, int TE, double gamma, double temperature, const double *prior_p, const double *rollout_p,
                            std::vector<double> &tab)
{
    UctTables o;
    o.cdf = (size_t)(H + 1); o.tpv = o.cdf + A; o.rcp = o.tpv + A; o.tpdiv = o.rcp + (size_t)(TE + 1);
    o.n = o.tpdiv + (size_t)A * (TE + 2);
    tab.resize(o.n);
    double *gpow = tab.data(), *cdf = gpow + o.cdf, *tpv = gpow + o.tpv, *rcp = gpow + o.rcp, *tpdiv = gpow + o.tpdiv;
    for (int h = 0; h <= H; ++h) gpow[h] = pow(gamma, (double)h);                 // gamma ** h
    double acc = 0.0;
    for (int a = 0; a < A; ++a) { acc += rollout_p ? rollout_p[a] : 1.0; cdf[a] = acc; } // numpy cumsum
    for (int a = 0; a < A; ++a) {
        // cdf /= cdf[-1]; Generator.choice(p=...): idx = searchsorted(cdf, u, 'right') with u = k * 2^-53, k < 2^53 integer;
        // cdf[a] <= u  <=>  ceil(cdf[a] * 2^53) <= k  (the scaling by 2^53 is exact)
        const double scaled = ceil(ldexp(cdf[a] / acc, 53));
        const uint64_t t = scaled >= 18446744073709551615.0 ? ~0ULL : (uint64_t)scaled;
        memcpy(&cdf[a], &t, sizeof(t));
    }
    rcp[0] = 0.0;
    for (int n = 1; n <= TE; ++n) rcp[n] = 1.0 / (double)n;                        // mcts.py:255  K / count, K = 1
    for (int a = 0; a < A; ++a) {
        const double tp = temperature * (double)A * (prior_p ? prior_p[a] : 0.0); // mcts.py:286, left to right
        tpv[a] = tp;
        tpdiv[(size_t)a * (TE + 2)] = 0.0;
        for (int n = 1; n <= TE + 1; ++n) tpdiv[(size_t)a * (TE + 2) + n] = tp / (double)n; // ... / (count + 1)
    }
    return o;
}

// ---- kept subtrees (step_strategy "subtree").  A plan continues the trees mp_uct_step_tree armed when its entry point's `cont`
// predicate holds.  A kept subtree only holds nodes created by the last `horizon` plans (a node at depth d survives d
// re-rootings and d <= horizon), so the stride stays O(horizon * episodes * |A|) however long the episode runs: kept_bound is
// the largest 1 + horizon * episodes * |A| of the plans since the last fresh tree, should the caller vary them.
// uct_kept_cap: the node stride of the continued trees, with room for this plan's expansions.  uct_fresh_tree: no tree is kept.
inline long uct_kept_cap(mp_ctx *ctx, int H, int E, int A)
{
    const long now = 1 + (long)H * E * A;
    if (now > ctx->tree.kept_bound) ctx->tree.kept_bound = now;
    const long bound = ctx->tree.kept_bound;
    return (ctx->tree.cap < bound ? (long)ctx->tree.cap : bound) + (long)E * A;
}

inline void uct_fresh_tree(mp_ctx *ctx, int H, int E, int A)
{
    ctx->tree.armed = false; ctx->tree.n_src = 0; ctx->tree.buf = 0;
    ctx->tree.kept_bound = 1 + (long)H * E * A;
}

// Apply the re-rooting armed by mp_uct_step_tree / mp_uct_step_tree_select: new tree i = the subtree under child actions[i] of
// the old root it continues (root i, or root source[i] of the tree.n_src old ones), written into the other tree workspace with
// node stride cap_new (>= the current tree sizes).  The sizes are updated in place, or -- with a selection -- written beside the
// sources and copied over the old ones when the kernel is done with them.  `launch(r)` starts the caller's kernel on the
// ctx's stream, from its current buffers into the other ones (reserved by the caller beforehand).
struct Reroot {
    int n_roots, n_src, A, cap_old, cap_new;
    int32_t *sizes, *sizes_new;
    const int32_t *src, *acts;
};

template <typename Launch>
inline int reroot_apply(mp_ctx *ctx, long cap_new, Launch launch)
{
    const int n_roots = ctx->tree.n_roots;
    const bool sel = ctx->tree.n_src > 0;
    // (a selection of more roots than the old batch: the sizes' slot grows now, keeping the old sizes the kernel reads)
    if (sel) MP_TRY(ws_reserve_keep(ctx, WS_TREE1, (size_t)n_roots * sizeof(int32_t)));
    int32_t *sizes = (int32_t *)ctx->ws[WS_TREE1].p, *fresh = (int32_t *)ctx->ws[WS_TREE7].p; // (fresh: [sources | new sizes])
    launch(Reroot{n_roots, sel ? ctx->tree.n_src : n_roots, ctx->tree.A, ctx->tree.cap, (int)cap_new, sizes, sel ? fresh + n_roots : sizes,
                  sel ? fresh : nullptr, (const int32_t *)ctx->ws[WS_TREE3].p});
    MP_HIP(hipGetLastError());
    if (sel) MP_TRY(reroot_sizes_back(ctx));
    ctx->tree.buf ^= 1;
    ctx->tree.cap = (int)cap_new;
    ctx->tree.armed = false;
    return MP_OK;
}

} // namespace mp
