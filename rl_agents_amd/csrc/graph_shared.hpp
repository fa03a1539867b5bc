// graph_shared.hpp -- what the two graph-based planners (gbopd.hip: GBOP-D, mp_gbopd_*; gbop.hip: GBOP, mp_gbop_*) share: one
// decision node per observed STATE with a lower and an upper bound of V, its parents in insertion order as a slice of the
// model's in-degrees, the backup ring, and the counters that outlive a plan.
//   host:   the handle's common part (GraphHandle: mp_gbopd and mp_gbop derive from it), the ring's capacity, the in-degree count
//           over a planner's own "states a listed (s, a) may lead to", the shared arrays, the refusals and the two knobs of a
//           plan call, the fields both args structs have (templates over the struct, as wave_mdp is: each keeps its layout, and
//           with it its kernels their register rows), and the head and the parent lists of an export;
//   device: the bounds between global memory and LDS, and what a refused planner is told.  They take values.
// A helper that reports takes the caller's name as `who`, one that reads the environment the knob's name.  Each planner keeps
// its expansion, backups, sampling rule, get_plan, launch geometry, the per-node loops of its export -- and get_node and the
// tail of a pop, which stay as each kernel wrote them (profiles/gbop_shared_refactor.md).
#pragma once
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "common.hpp"
#include "wave_host.hpp"

namespace mp {

// Pops one PLAN may make.  With accuracy 0 and rewards outside [0, 1] the bounds need not move monotonically and can cycle
// between neighbouring doubles for ever -- the reference then never returns; a device call must, and soon: the machine is
// shared.  The reference's longest measured plan made 490 000 pops; the limit is eight times that: a plan is ended when its
// NEXT pop would be pop number 2^22 + 1 (the outputs count the pops applied).  A planner's MAX_POPS knob lowers it (tests).
constexpr long kGraphMaxPops = 1L << 22;

struct GraphHandle {
    mp_ctx *ctx = nullptr;
    mp_model *model = nullptr;
    uint64_t model_serial = 0;
    int n = 0, S = 0, A = 0, qcap = 0;
    long E = 0;                 // parent entries per planner: in_ptr[S]
    double *lower = nullptr, *upper = nullptr;
    int32_t *index = nullptr, *npar = nullptr, *created = nullptr, *par = nullptr, *queue = nullptr;
    uint8_t *expanded = nullptr;
    int64_t *visits = nullptr, *n_obs = nullptr;
    int32_t *n_created = nullptr, *failed = nullptr, *root_of = nullptr;
    int32_t *in_ptr = nullptr;  // [S + 1], shared by the planners
    std::vector<int32_t> h_in_ptr;
    std::vector<mp_ctx::Block> blocks;
};

template <typename T>
inline hipError_t graph_alloc(GraphHandle *pl, T **out, size_t bytes)
{
    void *p = nullptr;
    size_t got = bytes;
    const hipError_t e = ctx_block_alloc(pl->ctx, &p, bytes ? bytes : 16, &got);
    if (e != hipSuccess) return e;
    pl->blocks.push_back({p, got});
    *out = static_cast<T *>(p);
    return hipSuccess;
}

template <typename Handle>
inline int graph_free(Handle *pl)
{
    if (!pl) return MP_OK;
    for (const auto &b : pl->blocks) ctx_block_release(pl->ctx, b.p, b.bytes);
    pl->blocks.clear();
    delete pl;
    return MP_OK;
}

// queue capacity: a power of two.  The argument, else the planner's environment knob, else 65 536 entries: the reference's list
// peaked at 19 243 on GBOP-D's golden cases, and with gamma 0.99, accuracy 1e-4 on a 50-state, 8-action model at 53 084 on a
// first plan and 62 751 on a following one -- within 4 % of the default.  While a batch's rings would exceed 4 GiB the default
// HALVES (16 384 at 65 536 planners) and no longer covers that configuration: such a batch names its queue_cap, or its hungry
// planners report MP_ERR_ALLOC.
inline int graph_queue_capacity(int queue_cap, const char *knob, int n_planners)
{
    long want = queue_cap;
    if (want <= 0) {
        if (const char *e = getenv(knob)) want = atol(e);
    }
    if (want <= 0) {
        want = 65536;
        while (want > 1024 && (size_t)want * 4 * (size_t)n_planners > ((size_t)4 << 30)) want >>= 1;
    }
    int q = 2;
    while (q < want && q < (1 << 28)) q <<= 1;
    return q;
}

// in-degrees: the distinct states with a listed action that may lead to c, into h_in_ptr and E.  successors(s, a, visit) calls
// visit(c) for every state c a listed (s, a) may lead to (for none where (s, a) is not listed) and hands back what it returns:
// MP_OK, or the refusal of a c outside the tables.
template <typename Successors>
inline int graph_count_parents(GraphHandle *pl, const char *who, Successors successors)
{
    const int S = pl->S, A = pl->A;
    pl->h_in_ptr.assign((size_t)S + 1, 0);
    std::vector<int32_t> last((size_t)S, -1);
    for (int s = 0; s < S; ++s)
        for (int a = 0; a < A; ++a)
            MP_TRY(successors(s, a, [&](int c) {
                if (c < 0 || c >= S) return fail(MP_ERR_ARG, "%s: a next state of (%d, %d) is %d: out of range", who, s, a, c);
                if (last[c] != s) { last[c] = s; ++pl->h_in_ptr[(size_t)c + 1]; }
                return (int)MP_OK;
            }));
    for (int s = 0; s < S; ++s) pl->h_in_ptr[(size_t)s + 1] += pl->h_in_ptr[s];
    pl->E = pl->h_in_ptr[S];
    return MP_OK;
}

// the shared arrays: allocated (else MP_ERR_ALLOC), cleared in stream order -- the blocks may be recycled ones -- and the
// in-degrees uploaded (else MP_ERR_HIP).  The caller adds its own arrays, words the failure and frees the handle.
inline int graph_create_shared(GraphHandle *pl)
{
    hipStream_t st = pl->ctx->stream;
    const size_t S = (size_t)pl->S, sn = S * pl->n, n = (size_t)pl->n;
    if (graph_alloc(pl, &pl->lower, sn * 8) != hipSuccess || graph_alloc(pl, &pl->upper, sn * 8) != hipSuccess ||
        graph_alloc(pl, &pl->index, sn * 4) != hipSuccess || graph_alloc(pl, &pl->npar, sn * 4) != hipSuccess ||
        graph_alloc(pl, &pl->created, sn * 4) != hipSuccess || graph_alloc(pl, &pl->expanded, sn) != hipSuccess ||
        graph_alloc(pl, &pl->visits, sn * 8) != hipSuccess || graph_alloc(pl, &pl->par, n * (size_t)pl->E * 4) != hipSuccess ||
        graph_alloc(pl, &pl->queue, n * (size_t)pl->qcap * 4) != hipSuccess || graph_alloc(pl, &pl->n_obs, n * 8) != hipSuccess ||
        graph_alloc(pl, &pl->n_created, n * 4) != hipSuccess || graph_alloc(pl, &pl->failed, n * 4) != hipSuccess ||
        graph_alloc(pl, &pl->root_of, n * 4) != hipSuccess || graph_alloc(pl, &pl->in_ptr, (S + 1) * 4) != hipSuccess)
        return MP_ERR_ALLOC;
    if (hipMemsetAsync(pl->index, 0xff, sn * 4, st) != hipSuccess || hipMemsetAsync(pl->npar, 0, sn * 4, st) != hipSuccess ||
        hipMemsetAsync(pl->created, 0, sn * 4, st) != hipSuccess || hipMemsetAsync(pl->expanded, 0, sn, st) != hipSuccess ||
        hipMemsetAsync(pl->visits, 0, sn * 8, st) != hipSuccess || hipMemsetAsync(pl->lower, 0, sn * 8, st) != hipSuccess ||
        hipMemsetAsync(pl->upper, 0, sn * 8, st) != hipSuccess || hipMemsetAsync(pl->n_obs, 0, n * 8, st) != hipSuccess ||
        hipMemsetAsync(pl->n_created, 0, n * 4, st) != hipSuccess || hipMemsetAsync(pl->failed, 0, n * 4, st) != hipSuccess ||
        hipMemsetAsync(pl->root_of, 0xff, n * 4, st) != hipSuccess ||
        hipMemcpyAsync(pl->in_ptr, pl->h_in_ptr.data(), (S + 1) * 4, hipMemcpyHostToDevice, st) != hipSuccess)
        return MP_ERR_HIP;
    return MP_OK;
}

// the refusals of a plan call, in two parts: a planner checks its own sizes between them, as it always has.  After wave_mem ...
inline int graph_check_handle(mp_ctx *ctx, const GraphHandle *pl, const char *who, const char *what_was_kept)
{
    if (pl->ctx != ctx) return fail(MP_ERR_ARG, "%s: planners belong to another context", who);
    if (pl->model->serial != pl->model_serial)
        return fail(MP_ERR_ARG, "%s: the model's tables or action sets changed under a kept graph (%s were built on the previous "
                                "tables): free the planners and create new ones", who, what_was_kept);
    return MP_OK;
}

// ... and the numbers no plan ends with: the reference never ends with a negative accuracy (every pop appends its parents) or
// with |gamma| >= 1, where the bounds grow for ever; a device call must end
inline int graph_check_numbers(const char *who, double gamma, double value_max, double accuracy)
{
    if (!(gamma > -1.0 && gamma < 1.0) || !(value_max == value_max) || !(accuracy >= 0.0))
        return fail(MP_ERR_ARG, "%s: need -1 < gamma < 1, accuracy >= 0 and a number for 1 / (1 - gamma)", who);
    return MP_OK;
}

// test knobs of a plan: a smaller pop limit (never a larger one), and the bytes of LDS up to which both bounds live there
// (16 KiB by default: ten planners per CU; 0: never)
inline long graph_max_pops(const char *knob)
{
    if (const char *e = getenv(knob)) {
        const long v = atol(e);
        if (v >= 1 && v < kGraphMaxPops) return v;
    }
    return kGraphMaxPops;
}

inline bool graph_use_lds(const char *knob, int S)
{
    size_t lds_limit = 16 * 1024;
    if (const char *e = getenv(knob)) lds_limit = (size_t)atol(e);
    if (lds_limit > 64 * 1024) lds_limit = 64 * 1024;
    return (size_t)S * 16 <= lds_limit;
}

// the fields GbArgs and GbopArgs share, from the handle and the call
template <typename Args>
inline void graph_args(const GraphHandle *pl, const char *max_pops_knob, double gamma, double value_max, double accuracy, Args *g)
{
    g->n = pl->n; g->S = pl->S; g->A = pl->A; g->qcap = pl->qcap; g->E = pl->E;
    g->max_pops = graph_max_pops(max_pops_knob);
    g->gamma = gamma; g->vmax = value_max; g->accuracy = accuracy;
    g->in_ptr = pl->in_ptr;
    g->lower = pl->lower; g->upper = pl->upper; g->index = pl->index; g->npar = pl->npar; g->created = pl->created; g->par = pl->par;
    g->queue = pl->queue; g->n_created = pl->n_created; g->failed = pl->failed; g->root_of = pl->root_of; g->expanded = pl->expanded;
    g->visits = pl->visits; g->n_obs = pl->n_obs;
}

// the six results both planners report, in the workspace slots they have always had (WS_IO3, the plan, has each planner's shape)
template <typename Args>
inline void graph_results_io(WaveIo &io, int32_t *plan_len, int32_t *status, int64_t *env_steps, int64_t *pops, double *value_lower,
                             double *value_upper, Args *g)
{
    io.add(WS_IO4, plan_len, &g->plan_len);
    io.add(WS_IO5, status, &g->status);
    io.add(WS_IO6, env_steps, &g->env_steps);
    io.add(WS_IO7, pops, &g->pops);
    io.add(WS_IO8, value_lower, &g->root_lower);
    io.add(WS_IO9, value_upper, &g->root_upper);
}

// ---- export.  The host copies of one planner's per-state arrays, in creation order through `created`.
struct GraphExport {
    int32_t n_nodes = 0, root_state = -1;
    std::vector<double> lower, upper;
    std::vector<int32_t> index, npar, created, par;
    std::vector<uint8_t> expanded;
};

// every check of an export, its three scalars, the copies of the shared arrays and `visits` / `root`
inline int graph_export_begin(const GraphHandle *pl, const char *who, const char *no_longer, int planner, int cap, int32_t *n_nodes,
                              int64_t *visits, int64_t *n_observations, int32_t *root, GraphExport *x)
{
    if (!pl || !n_nodes) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    if (planner < 0 || planner >= pl->n) return fail(MP_ERR_ARG, "%s: planner %d out of range", who, planner);
    if (pl->model->serial != pl->model_serial)
        return fail(MP_ERR_ARG, "%s: the model's tables or action sets changed under a kept graph: the %s of its nodes are no longer "
                                "the model's", who, no_longer);
    MP_HIP(hipSetDevice(pl->ctx->device));
    MP_HIP(hipStreamSynchronize(pl->ctx->stream));
    const size_t S = (size_t)pl->S, E = (size_t)pl->E, r = (size_t)planner;
    int64_t nobs = 0;
    MP_HIP(hipMemcpy(&x->n_nodes, pl->n_created + r, 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(&x->root_state, pl->root_of + r, 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(&nobs, pl->n_obs + r, 8, hipMemcpyDeviceToHost));
    if (x->n_nodes < 0 || (size_t)x->n_nodes > S) return fail(MP_ERR_ARG, "%s: bad node count %d", who, x->n_nodes);
    *n_nodes = x->n_nodes;
    if (n_observations) *n_observations = nobs;
    if (cap < x->n_nodes) return fail(MP_ERR_ARG, "%s: capacity %d < %d nodes", who, cap, x->n_nodes);
    x->lower.resize(S); x->upper.resize(S); x->index.resize(S); x->npar.resize(S); x->created.resize(S); x->expanded.resize(S);
    x->par.resize(E);
    MP_HIP(hipMemcpy(x->lower.data(), pl->lower + r * S, S * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(x->upper.data(), pl->upper + r * S, S * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(x->index.data(), pl->index + r * S, S * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(x->npar.data(), pl->npar + r * S, S * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(x->created.data(), pl->created + r * S, S * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(x->expanded.data(), pl->expanded + r * S, S, hipMemcpyDeviceToHost));
    if (E) MP_HIP(hipMemcpy(x->par.data(), pl->par + r * E, E * 4, hipMemcpyDeviceToHost));
    if (visits) MP_HIP(hipMemcpy(visits, pl->visits + r * S, S * 8, hipMemcpyDeviceToHost));
    if (root) *root = x->root_state >= 0 && (size_t)x->root_state < S ? x->index[(size_t)x->root_state] : -1;
    return MP_OK;
}

// the parents of node i (state s) as creation indices behind *np_total, never past the state's slice; parent_ptr[i + 1] closes it
inline void graph_export_parents(const GraphHandle *pl, const GraphExport &x, int32_t i, int32_t s, int32_t *parent_ptr,
                                 int32_t *parent_idx, int32_t *np_total)
{
    const int32_t base = pl->h_in_ptr[(size_t)s], room = pl->h_in_ptr[(size_t)s + 1] - base;
    const int32_t np = x.npar[(size_t)s] < room ? x.npar[(size_t)s] : room;
    for (int32_t j = 0; j < np; ++j) {
        const int32_t ps = x.par[(size_t)base + j];
        if (parent_idx) parent_idx[*np_total] = ps >= 0 && ps < pl->S ? x.index[(size_t)ps] : -1;
        ++*np_total;
    }
    if (parent_ptr) parent_ptr[i + 1] = *np_total;
}

// ---- device.  A workgroup is one wavefront: every __syncthreads is the wait for the wave's own stores.

// what a planner that failed for good in an earlier call, or whose root is outside the tables, is told (lane 0)
__device__ __forceinline__ void graph_refuse(int r, int status, int32_t *plan_len, int32_t *status_out, double *root_lower,
                                             double *root_upper, int64_t *env_steps, int64_t *pops)
{
    if (plan_len) plan_len[r] = 0;
    if (status_out) status_out[r] = status;
    if (root_lower) root_lower[r] = 0.0;
    if (root_upper) root_upper[r] = 0.0;
    if (env_steps) env_steps[r] = 0;
    if (pops) pops[r] = 0;
}

// both bounds of the created states from the planner's global arrays into LDS, and back
__device__ __forceinline__ void graph_stage_in(const double *g_lower, const double *g_upper, long sb, const int32_t *created, int n_created,
                                               double *lower, double *upper, int lane)
{
    for (int i = lane; i < n_created; i += 64) {
        const int s = created[i];
        lower[s] = g_lower[sb + s];
        upper[s] = g_upper[sb + s];
    }
    __syncthreads();
}

__device__ __forceinline__ void graph_write_back(double *g_lower, double *g_upper, long sb, const int32_t *created, int n_created,
                                                 const double *lower, const double *upper, int lane)
{
    __syncthreads();
    for (int i = lane; i < n_created; i += 64) {
        const int s = created[i];
        g_lower[sb + s] = lower[s];
        g_upper[sb + s] = upper[s];
    }
}

} // namespace mp
