// gape_shared.hpp -- what the two MDP-GapE translation units (gape.hip: mp_gape_plan / mp_gape_plan_models; gape_stoch.hip:
// mp_gape_plan_stochastic) share besides the selection helpers of gape_select.hpp, which this header brings along.
//   host:   the nine result arrays of a call (GapeResults: a member of both args structs, registered with a WaveIo by one function),
//           the argument checks, the two capacity refusals, and the packing and upload of the host tables;
//   device: the stopping rule and the read-out of a root, the latter a template over small accessors, as gape_first_max: each
//           kernel keeps its own record (GapeNode, GsNode) and says how a field of it is read.
// The episode loop stays with each kernel whole -- the walk, the listing of an expansion, the deferred reward bounds, the backup:
// shared, the listing and the bound loop left every resource row as it was but not the kernel times (profiles/
// gape_shared_refactor.md) -- and so do the two tree exports.
#pragma once
#include <math.h>

#include <vector>

#include "common.hpp"
#include "gape_select.hpp"
#include "pcg64.hpp"
#include "wave_host.hpp"

namespace mp {

constexpr size_t kGapeKeepBytes = (size_t)1 << 30; // trees of every root kept while they fit (the rule of OLOP and BRUE)

// the result arrays of a plan call, the caller's or their device side; any may be NULL (not asked for)
struct GapeResults {
    int32_t *plans, *plan_len, *episodes_run, *status, *arms; // arms [n_roots][2]: the best arm's action and the challenger's
    int64_t *env_steps, *child_count;  // child_count [n_roots][A] by column, -1 where the root lists no such action
    double *child_lower, *child_upper; // [n_roots][A]
};

inline void gape_results_io(WaveIo &io, const GapeResults &host, GapeResults *dev, int max_plan_len, int A)
{
    io.add(WS_IO3, host.plans, &dev->plans, (size_t)max_plan_len);
    io.add(WS_IO4, host.plan_len, &dev->plan_len);
    io.add(WS_IO5, host.episodes_run, &dev->episodes_run);
    io.add(WS_IO8, host.env_steps, &dev->env_steps);
    io.add(WS_IO7, host.status, &dev->status);
    io.add(WS_IO6, host.child_lower, &dev->child_lower, (size_t)A);
    io.add(WS_IO9, host.child_upper, &dev->child_upper, (size_t)A);
    io.add(WS_IO1, host.child_count, &dev->child_count, (size_t)A);
    io.add(WS_IO10, host.arms, &dev->arms, (size_t)2);
}

// the host tables of a call and, after gape_upload_tables, their device side: thresholds by count [M + 2] (tthr: those of the
// transition bound, NULL for mp_gape_plan), the initial values [H + 1], the columns of the environment's actions [n_env].  `col`
// is filled on the device side only: the host's columns are the caller's int32 `action_column` (NULL: the identity), which
// gape_check_args and gape_upload_tables take beside the bundle.
struct GapeTables {
    const double *thr, *tthr, *vinit;
    const double *col; // (small integers, kept in the double table)
};

// the checks both entry points make of their sizes, scalars and tables (`max_horizon`: the path of an episode fits LDS)
inline int gape_check_args(const char *who, int n_roots, int episodes, int horizon, int max_horizon, int max_plan_len, int A,
                           int n_actions_env, double gamma, double accuracy, const GapeTables &t, int continuation,
                           const int32_t *action_column)
{
    if (n_roots < 1 || episodes < 0 || horizon < 1 || horizon > max_horizon || max_plan_len < 0 || A < 1 || n_actions_env < 1)
        return fail(MP_ERR_ARG, "%s: bad sizes", who);
    // a NaN among them would make NaN bounds of every node, which the reference plans on and no plan is worth
    if (!isfinite(gamma) || !isfinite(accuracy)) return fail(MP_ERR_ARG, "%s: gamma and accuracy must be finite", who);
    for (int c = 0; c < episodes + 2; ++c) {
        if (!isfinite(t.thr[c])) return fail(MP_ERR_ARG, "%s: the threshold of count %d is not finite", who, c + 1);
        if (t.tthr && !isfinite(t.tthr[c])) return fail(MP_ERR_ARG, "%s: the transition threshold of count %d is not finite", who, c + 1);
    }
    for (int d = 0; d <= horizon; ++d)
        if (!isfinite(t.vinit[d])) return fail(MP_ERR_ARG, "%s: the initial value of depth %d is not finite", who, d);
    if (continuation != 0 && continuation != 1) return fail(MP_ERR_ARG, "%s: continuation %d is neither 0 (action 0) nor 1 (uniform)", who, continuation);
    if (!action_column && n_actions_env != A)
        return fail(MP_ERR_ARG, "%s: %d environment actions need their columns among the model's %d", who, n_actions_env, A);
    for (int a = 0; action_column && a < n_actions_env; ++a)
        if (action_column[a] < -1 || action_column[a] >= A) return fail(MP_ERR_ARG, "%s: column %d out of range", who, action_column[a]);
    return MP_OK;
}

// a tree of `cap` records of `node_bytes` and two values each must be indexable and fit the workspace of one root
inline int gape_check_capacity(const char *who, long long cap, size_t node_bytes)
{
    if (cap > 0x7fffffffLL) return fail(MP_ERR_ARG, "%s: %lld nodes per tree do not fit a 32-bit index", who, cap);
    if ((size_t)cap * (node_bytes + 2 * sizeof(double)) > kGapeKeepBytes)
        return fail(MP_ERR_ARG, "%s: %lld nodes per tree take more than 1 GiB", who, cap);
    return MP_OK;
}

// one table -- thr, tthr (where there is one), vinit, col -- uploaded as tables of kind `kind`; *dev points into it
inline int gape_upload_tables(mp_ctx *ctx, int kind, int episodes, int horizon, int n_actions_env, const int32_t *action_column,
                              const GapeTables &host, GapeTables *dev)
{
    const size_t M2 = (size_t)episodes + 2, n_thr = host.tthr ? 2 * M2 : M2;
    std::vector<double> tab(n_thr + horizon + 1 + n_actions_env);
    for (size_t c = 0; c < M2; ++c) {
        tab[c] = host.thr[c];
        if (host.tthr) tab[M2 + c] = host.tthr[c];
    }
    for (int d = 0; d <= horizon; ++d) tab[n_thr + d] = host.vinit[d];
    for (int a = 0; a < n_actions_env; ++a) tab[n_thr + horizon + 1 + a] = action_column ? action_column[a] : a;
    double *d_tab = nullptr;
    MP_TRY(upload_tables(ctx, kind, tab, &d_tab));
    dev->thr = d_tab; dev->tthr = host.tthr ? d_tab + M2 : nullptr; dev->vinit = d_tab + n_thr; dev->col = dev->vinit + horizon + 1;
    return MP_OK;
}

// the stopping rule (mdp_gape.py:100-102) on the root's k0 arms, whose values lie from record fc0 on: the best arm and the
// challenger anew, and whether the challenger's upper value is within `accuracy` of the best arm's lower one
__device__ __forceinline__ bool gape_stop(const double *V, int fc0, int k0, int lane, double accuracy, int *best, int *challenger)
{
    int sel;
    gape_bai(V + 2 * (long)fc0, k0, lane, &sel, best, challenger);
    return V[2 * (long)(fc0 + *challenger)] - V[2 * (long)(fc0 + *best) + 1] < accuracy;
}

// get_plan (mdp_gape.py:129-131) and what the caller is told of root `root`: the [A] rows reset and the root's k0 arms (records
// fc0 ..) written by column, then by lane 0 the generator, the plan -- the best arm's action -- the arms and the counters.
// `action(i)` / `count(i)` read the i-th arm's record.  The caller synchronises before (the arms' values are final) and after.
template <typename Action, typename Count>
__device__ __forceinline__ void gape_read_out(const GapeResults &o, uint64_t *rng, int root, int A, int max_plan_len, int lane,
                                              const double *V, int fc0, int k0, const Pcg64 &gen, int status, int best,
                                              int challenger, int episodes_run, long steps, Action action, Count count)
{
    for (int a = lane; a < A; a += 64) {
        if (o.child_count) o.child_count[(long)root * A + a] = -1;
        if (o.child_lower) o.child_lower[(long)root * A + a] = 0.0;
        if (o.child_upper) o.child_upper[(long)root * A + a] = 0.0;
    }
    __syncthreads();
    for (int i = lane; i < k0; i += 64) {
        const int a = action(i);
        if (o.child_count) o.child_count[(long)root * A + a] = count(i);
        if (o.child_lower) o.child_lower[(long)root * A + a] = V[2 * (long)(fc0 + i) + 1];
        if (o.child_upper) o.child_upper[(long)root * A + a] = V[2 * (long)(fc0 + i)];
    }
    if (lane == 0) {
        const bool ok = status == MP_OK && best >= 0;
        gen.store(rng + (long)root * 6);
        if (o.plans)
            for (int i = 0; i < max_plan_len; ++i) o.plans[(long)root * max_plan_len + i] = ok && i == 0 ? action(best) : -1;
        if (o.plan_len) o.plan_len[root] = ok ? 1 : 0;
        if (o.episodes_run) o.episodes_run[root] = episodes_run;
        if (o.status) o.status[root] = status;
        if (o.env_steps) o.env_steps[root] = steps;
        if (o.arms) {
            o.arms[2 * (long)root] = ok ? action(best) : -1;
            o.arms[2 * (long)root + 1] = ok ? action(challenger) : -1;
        }
    }
}

} // namespace mp
