// gbopd.hip -- GBOP-D, graph-based optimistic planning for deterministic systems (tree_search/graph_based.py), for many
// independent planners of one deterministic table model.
//
// The reference's GraphBasedPlanner merges the nodes that share an observation into ONE node per state (get_node, :110-116),
// keeps a lower and an upper bound of V per node (GraphNode.__init__, :12-20) and, after every expansion (:39-53), tightens
// them with a partial value iteration that runs backwards through the graph (:66-78): a first-in-first-out list that holds
// duplicates; a popped node takes max_a r(a) + gamma * bound(child a) for both bounds and, when either moved by more than
// `accuracy`, appends all its parents.  planner.nodes, updates_count and observations outlive plan() calls (reset(), :93-94,
// only replaces `root`), so the planner state is a device-resident handle, as mp_saopd is.
//
// Mapping.  One planner per WAVEFRONT (a workgroup is one wavefront).  The chain of pops is serial by the reference's
// definition (Gauss-Seidel: a pop reads the bounds earlier pops wrote), so the order-dependent parts run as uniform code and
// the lanes cover what is independent inside a step, 64 at a time with no limit at 64:
//   a node's actions      the model row read of an expansion, both bound reductions of a pop (wave_max), the optimistic argmax
//                         with its tie draw (sampling_rule, :22-30) and the conservative first maximum (selection_rule, :32-37)
//   a node's parents      the append of a popped node's parents to the queue (:78)
//   an expansion's slots  the duplicate check of `parents.add` (:51): two actions of one expansion may lead to the same child
//
// Storage, per planner, addressed by STATE (a finite MDP's graph never holds more than S nodes):
//   lower / upper f64 [S]     value_lower / value_upper;  index i32 [S]  creation index (position in planner.nodes), -1 = absent
//   expanded u8 [S]           "node.children is not empty";  created i32 [S]  the states in creation order (for the export)
//   visits / updates i64 [S]  lifetime counters: get_visits() (abstract.py:163-167) and updates_count (:69)
//   par i32 [E], npar i32 [S] the parents of a node in INSERTION order.  A node s is expanded once in a planner's lifetime, so
//                             parents[c] can only ever hold the distinct states with a listed action into c: the handle counts
//                             them on the model once (in_ptr [S + 1], shared by the planners) and every node's list is a
//                             contiguous slice of E = in_ptr[S] <= S * A entries -- lanes read it 64 parents per load
//   queue i32 [queue_cap]     the backup queue: a ring of state indices with duplicates.  A planner whose ring fills up
//                             reports MP_ERR_ALLOC and stays failed (its bounds are half updated); the others are unaffected
// While 16 * S bytes fit (MP_GBOPD_LDS_BYTES, default 16 KiB) both bounds live in LDS for the plan: the hop "child's bound"
// of every pop and every descent step is then an LDS read.  They are staged in from / written back to global memory for the
// created states only.
//
// What bounds a pop: the dependent chain  queue front (global) -> model row + the children's bounds -> wave_max (two DPP
// reductions) -> compare with the old bounds -> store -> parents appended behind the tail.  Nothing of pop k + 1 can start
// before pop k has stored: the next front may be the node just written, or read it as a child.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "common.hpp"
#include "opd_closing.hpp"
#include "pcg64.hpp"
#include "wave.hpp"
#include "wave_host.hpp"

struct mp_gbopd {
    mp_ctx *ctx = nullptr;
    mp_model *model = nullptr;
    uint64_t model_serial = 0;
    int n = 0, S = 0, A = 0, qcap = 0;
    long E = 0;                 // parent entries per planner: in_ptr[S]
    double *lower = nullptr, *upper = nullptr;
    int32_t *index = nullptr, *npar = nullptr, *created = nullptr, *par = nullptr, *queue = nullptr;
    uint8_t *expanded = nullptr;
    int64_t *visits = nullptr, *updates = nullptr, *n_obs = nullptr;
    int32_t *n_created = nullptr, *failed = nullptr, *root_of = nullptr;
    int32_t *in_ptr = nullptr;  // [S + 1], shared
    std::vector<mp::Rec> hrec;  // host copy of the model's records (in-degrees at creation, children / rewards of the export)
    std::vector<int32_t> h_in_ptr;
    std::vector<mp_ctx::Block> blocks;
};

namespace mp {

struct GbArgs {
    int n, S, A, K, timeout, qcap;
    long E, max_pops;
    double gamma, vmax, accuracy;
    const Rec *rec;
    const int32_t *in_ptr;
    const int32_t *root_state;
    uint64_t *rng;
    double *lower, *upper;
    int32_t *index, *npar, *created, *par, *queue, *n_created, *failed, *root_of;
    uint8_t *expanded;
    int64_t *visits, *updates, *n_obs;
    int32_t *plans, *plan_len, *status;
    double *root_lower, *root_upper;
    int64_t *env_steps, *n_updates;
};

// Pops one PLAN may make.  With accuracy 0 and rewards outside [0, 1] the bounds need not move monotonically and can cycle
// between neighbouring doubles for ever -- the reference then never returns; a device call must, and soon: the machine is
// shared.  The reference's longest measured plan made 490 000 pops; the limit is eight times that: a plan is ended when its
// NEXT pop would be pop number 2^22 + 1 (the outputs count the pops applied).  MP_GBOPD_MAX_POPS lowers it (tests).
constexpr long kGbMaxPops = 1L << 22;

template <bool LDSV>
__global__ __launch_bounds__(64) void gbopd_kernel(GbArgs p)
{
    extern __shared__ __attribute__((aligned(16))) double lds_v[];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int S = p.S, A = p.A, T = p.timeout;
    const long sb = (long)r * S;
    const bool l0 = lane == 0;
    const double ninf = -INFINITY;
    const unsigned long long lt_mask = (1ULL << lane) - 1ULL;

    const int s0 = p.root_state[r];
    int status = p.failed[r]; // failed for good in an earlier call: the code it failed with
    if (status == MP_OK && (unsigned)s0 >= (unsigned)S) status = MP_ERR_ARG;
    if (status != MP_OK) {
        if (p.plans)
            for (int i = lane; i < T; i += 64) p.plans[(long)r * T + i] = -1;
        if (l0) {
            if (p.plan_len) p.plan_len[r] = 0;
            if (p.status) p.status[r] = status;
            if (p.root_lower) p.root_lower[r] = 0.0;
            if (p.root_upper) p.root_upper[r] = 0.0;
            if (p.env_steps) p.env_steps[r] = 0;
            if (p.n_updates) p.n_updates[r] = 0;
        }
        return;
    }
    double *const lower = LDSV ? lds_v : p.lower + sb;
    double *const upper = LDSV ? lds_v + S : p.upper + sb;
    int32_t *const index = p.index + sb, *const npar = p.npar + sb, *const created = p.created + sb;
    uint8_t *const expanded = p.expanded + sb;
    int64_t *const visits = p.visits + sb, *const updates = p.updates + sb;
    int32_t *const par = p.par + (long)r * p.E;
    int32_t *const queue = p.queue + (long)r * p.qcap;
    const unsigned qmask = (unsigned)p.qcap - 1u;
    const Rec *const rec = p.rec;
    const double gamma = p.gamma;

    int n_created = p.n_created[r];
    if (LDSV) { // stage in the bounds of the nodes that exist
        for (int i = lane; i < n_created; i += 64) {
            const int s = created[i];
            lower[s] = p.lower[sb + s];
            upper[s] = p.upper[sb + s];
        }
        __syncthreads();
    }
    // plan(), :119: root = get_node(observation)
    if (index[s0] < 0) {
        if (l0) {
            index[s0] = n_created; created[n_created] = s0;
            lower[s0] = 0.0; upper[s0] = p.vmax;
        }
        ++n_created;
    }
    if (l0) p.root_of[r] = s0;
    // (every __syncthreads of this kernel: stores of this wave followed by loads of its other lanes; the workgroup is one
    // wavefront, so the barrier is the wait for its own stores)
    __syncthreads();

    Pcg64 gen;
    gen.load(p.rng + (long)r * 6);
    long steps = 0, pops_total = 0;

    for (int epoch = 0; epoch < p.K && status == MP_OK; ++epoch) {
        // ---- run(), :96-108
        int node = s0;
        bool sink = false;
        for (int k = 0; k < T; ++k) {
            if (expanded[node]) {
                // sampling_rule (:22-30): random_argmax over r(a) + gamma * child.value_upper in key order = listing order
                {
                    double m = ninf;
                    for (int a = lane; a < A; a += 64) {
                        const Rec rc = rec[(long)node * A + a];
                        if (rc.flags & 4u) {
                            const double q = rc.reward + gamma * upper[rc.next];
                            m = q > m ? q : m;
                        }
                    }
                    m = wave_max(m);
                    // (one maximum: the generator does not advance)
                    const int a = draw_tie_chunks(A, [&](int b) {
                        const Rec rc = rec[(long)node * A + b];
                        return (rc.flags & 4u) != 0 && rc.reward + gamma * upper[rc.next] == m; }, gen);
                    node = __builtin_amdgcn_readfirstlane(rec[(long)node * A + a].next);
                }
                // (never follow a record outside the tables: NaN rewards leave no maximum to pick)
                if ((unsigned)node >= (unsigned)S) { status = MP_ERR_ARG; sink = true; break; }
                continue;
            }
            // ---- expand (:39-53): the listed actions in listing order, 64 per trip
            sink = true;
            const int s = node;
            bool any_valid = false, bad = false;
            for (int a0 = 0; a0 < A; a0 += 64) {
                const int a = a0 + lane;
                bool valid = false;
                int c = 0;
                if (a < A) {
                    const Rec rc = rec[(long)s * A + a];
                    valid = (rc.flags & 4u) != 0;
                    c = rc.next;
                }
                const unsigned long long vmask = ballot64(valid);
                // parents is a SET: an earlier slot of this trip with the same child ...
                bool dup = false;
                const int lim = A - a0 < 64 ? A - a0 : 64;
                for (int k2 = 0; k2 < lim; ++k2) {
                    const int ck = __builtin_amdgcn_readlane(c, k2);
                    if (((vmask >> k2) & 1ULL) && k2 < lane && ck == c) dup = true;
                }
                // ... or of an earlier trip: s expands once in the planner's lifetime, so if parents[c] holds s it is its last entry
                int idx = -1, np = 0, base = 0, room = 0;
                if (valid && !dup) {
                    idx = index[c]; np = npar[c];
                    base = p.in_ptr[c]; room = p.in_ptr[c + 1] - base;
                    if (np > 0 && np <= room && par[base + np - 1] == s) dup = true;
                }
                const bool first = valid && !dup;
                const bool create = first && idx < 0; // get_node (:110-116): the next creation index, in key order
                const unsigned long long cmask = ballot64(create);
                if (create) {
                    const int ni = n_created + __popcll(cmask & lt_mask);
                    index[c] = ni; created[ni] = c;
                    lower[c] = 0.0; upper[c] = p.vmax;
                }
                n_created += __popcll(cmask);
                if (first) {
                    if (np < room) { par[base + np] = s; npar[c] = np + 1; }
                    else bad = true; // (the model's tables changed under a kept graph: never write past the slice)
                }
                if (valid) atomicAdd(reinterpret_cast<unsigned long long *>(&visits[c]), 1ULL); // planner.step, abstract.py:158-161
                steps += __popcll(vmask);
                any_valid = any_valid || vmask != 0ULL;
                __syncthreads();
            }
            if (l0) expanded[s] = any_valid ? 1 : 0;
            if (any64(bad)) { status = MP_ERR_ARG; break; }
            // a node no action is listed for: the reference's np.amax([]) raises ValueError in partial_value_iteration (:74)
            if (!any_valid) { status = MP_ERR_GBOPD_NO_ACTION; break; }
            // ---- partial_value_iteration (:66-78)
            unsigned qh = 0, qt = 1;
            if (l0) queue[0] = s;
            __syncthreads();
            long pops = 0;
            while (qh != qt) {
                const int v = __builtin_amdgcn_readfirstlane(queue[qh & qmask]);
                if (pops_total + pops >= p.max_pops) { status = MP_ERR_GBOPD_DIVERGED; break; } // (see kGbMaxPops: the front stays unpopped)
                ++qh; ++pops;
                const double old_l = lower[v], old_u = upper[v];
                const int np = npar[v], base = p.in_ptr[v];
                double bl = ninf, bu = ninf;
                for (int a = lane; a < A; a += 64) {
                    const Rec rc = rec[(long)v * A + a];
                    if (rc.flags & 4u) {
                        const double ql = rc.reward + gamma * lower[rc.next], qu = rc.reward + gamma * upper[rc.next];
                        bl = ql > bl ? ql : bl;
                        bu = qu > bu ? qu : bu;
                    }
                }
                bl = wave_max(bl);
                bu = wave_max(bu);
                double delta = 0.0;
                const double dl = fabs(old_l - bl), du = fabs(old_u - bu);
                if (dl > delta) delta = dl;
                if (du > delta) delta = du;
                if (l0) { lower[v] = bl; upper[v] = bu; }
                if (delta > p.accuracy) { // queue.extend(list(node.parents)), insertion order
                    if (qt - qh + (unsigned)np > (unsigned)p.qcap) { status = MP_ERR_ALLOC; break; }
                    for (int j = lane; j < np; j += 64) queue[(qt + (unsigned)j) & qmask] = par[base + j];
                    qt += (unsigned)np;
                }
                __syncthreads();
            }
            if (l0) updates[s] += pops; // :69 counts on the EXPANDED node
            pops_total += pops;
            break;
        }
        if (!sink && status == MP_OK) { // for ... else (:106-108): n copies of the last node's observation
            steps += A;
            // (an atomic like the expansions' increments: those execute in L2, and a plain read-modify-write could read a stale L1 line)
            if (l0) atomicAdd(reinterpret_cast<unsigned long long *>(&visits[node]), (unsigned long long)A);
        }
    }
    // ---- get_plan (:126-135) with selection_rule (:32-37): Python max, the FIRST maximum in key order, no draw
    int len = 0;
    if (status == MP_OK) {
        __syncthreads();
        int node = s0;
        for (int i = 0; i < T; ++i) {
            if (!expanded[node]) break;
            int a = 0;
            {
                double m = ninf;
                for (int b = lane; b < A; b += 64) {
                    const Rec rc = rec[(long)node * A + b];
                    if (rc.flags & 4u) {
                        const double q = rc.reward + gamma * lower[rc.next];
                        m = q > m ? q : m;
                    }
                }
                m = wave_max(m);
                for (int b0 = 0; b0 < A; b0 += 64) {
                    const int b = b0 + lane;
                    bool hit = false;
                    if (b < A) {
                        const Rec rc = rec[(long)node * A + b];
                        hit = (rc.flags & 4u) != 0 && rc.reward + gamma * lower[rc.next] == m;
                    }
                    const unsigned long long best = ballot64(hit);
                    if (best) { a = b0 + __ffsll((long long)best) - 1; break; }
                }
                node = __builtin_amdgcn_readfirstlane(rec[(long)node * A + a].next);
            }
            if ((unsigned)node >= (unsigned)S) { status = MP_ERR_ARG; len = 0; break; }
            if (l0 && p.plans) p.plans[(long)r * T + len] = a;
            ++len;
        }
    }
    if (p.plans)
        for (int i = len + lane; i < T; i += 64) p.plans[(long)r * T + i] = -1;
    const double root_l = lower[s0], root_u = upper[s0];
    if (LDSV) { // write the bounds back
        __syncthreads();
        for (int i = lane; i < n_created; i += 64) {
            const int s = created[i];
            p.lower[sb + s] = lower[s];
            p.upper[sb + s] = upper[s];
        }
    }
    if (l0) {
        gen.store(p.rng + (long)r * 6);
        p.n_created[r] = n_created;
        p.n_obs[r] += steps;
        if (status != MP_OK) p.failed[r] = status; // sticky: the graph is half updated
        if (p.plan_len) p.plan_len[r] = len;
        if (p.status) p.status[r] = status;
        if (p.root_lower) p.root_lower[r] = root_l;
        if (p.root_upper) p.root_upper[r] = root_u;
        if (p.env_steps) p.env_steps[r] = steps;
        if (p.n_updates) p.n_updates[r] = pops_total;
    }
}

template <typename T>
static hipError_t gb_alloc(mp_gbopd *pl, T **out, size_t bytes)
{
    void *p = nullptr;
    size_t got = bytes;
    const hipError_t e = ctx_block_alloc(pl->ctx, &p, bytes ? bytes : 16, &got);
    if (e != hipSuccess) return e;
    pl->blocks.push_back({p, got});
    *out = static_cast<T *>(p);
    return hipSuccess;
}

} // namespace mp

using namespace mp;

extern "C" {

int mp_gbopd_free(mp_gbopd *pl)
{
    if (!pl) return MP_OK;
    for (const auto &b : pl->blocks) ctx_block_release(pl->ctx, b.p, b.bytes);
    pl->blocks.clear();
    delete pl;
    return MP_OK;
}

int mp_gbopd_create(mp_ctx *ctx, mp_model *model, int32_t n_planners, int32_t queue_cap, mp_gbopd **out)
{
    if (!ctx || !model || !out) return fail(MP_ERR_ARG, "mp_gbopd_create: NULL argument");
    if (model->mode != MP_MODE_DETERMINISTIC || !model->rec)
        return fail(MP_ERR_MODE, "mp_gbopd_create: GBOP-D needs a deterministic table model (mode %d)", model->mode);
    if (model->M != 1 || model->NB != 1)
        return fail(MP_ERR_MODE, "mp_gbopd_create: one whole model expected (no joint or batch model)");
    if (n_planners < 1 || model->S < 1 || model->A < 1) return fail(MP_ERR_ARG, "mp_gbopd_create: n_planners = %d", n_planners);
    MP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    mp_gbopd *pl = new (std::nothrow) mp_gbopd;
    if (!pl) return fail(MP_ERR_ALLOC, "mp_gbopd_create: out of memory");
    pl->ctx = ctx; pl->model = model; pl->model_serial = model->serial; pl->n = n_planners; pl->S = model->S; pl->A = model->A;
    const int S = pl->S, A = pl->A;
    // queue capacity: a power of two.  Default 65 536 entries: the reference's list peaked at 19 243 on the golden cases, and
    // with gamma 0.99, accuracy 1e-4 on a 50-state, 8-action model at 53 084 on a first plan and 62 751 on a following one --
    // within 4 % of the default.  While a batch's rings would exceed 4 GiB the default HALVES (16 384 at 65 536 planners) and
    // no longer covers that configuration: such a batch names its queue_cap, or its hungry planners report MP_ERR_ALLOC.
    long want = queue_cap;
    if (want <= 0) {
        if (const char *e = getenv("MP_GBOPD_QUEUE")) want = atol(e);
    }
    if (want <= 0) {
        want = 65536;
        while (want > 1024 && (size_t)want * 4 * (size_t)n_planners > ((size_t)4 << 30)) want >>= 1;
    }
    int q = 2;
    while (q < want && q < (1 << 28)) q <<= 1;
    pl->qcap = q;
    // the model's records on the host; in-degrees: the distinct states with a listed action into c
    pl->hrec.resize((size_t)S * A);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(pl->hrec.data(), model->rec, (size_t)S * A * sizeof(Rec), hipMemcpyDeviceToHost) != hipSuccess) {
        delete pl;
        return fail(MP_ERR_HIP, "mp_gbopd_create: reading the model's records failed");
    }
    pl->h_in_ptr.assign((size_t)S + 1, 0);
    {
        std::vector<int32_t> last((size_t)S, -1);
        for (int s = 0; s < S; ++s)
            for (int a = 0; a < A; ++a) {
                const Rec &rc = pl->hrec[(size_t)s * A + a];
                if (!(rc.flags & 4u)) continue;
                if (rc.next < 0 || rc.next >= S) {
                    delete pl;
                    return fail(MP_ERR_ARG, "mp_gbopd_create: transition[%d, %d] = %d out of range", s, a, rc.next);
                }
                if (last[rc.next] != s) { last[rc.next] = s; ++pl->h_in_ptr[(size_t)rc.next + 1]; }
            }
        for (int s = 0; s < S; ++s) pl->h_in_ptr[(size_t)s + 1] += pl->h_in_ptr[s];
    }
    pl->E = pl->h_in_ptr[S];
    const size_t sn = (size_t)S * pl->n, n = (size_t)pl->n;
    if (gb_alloc(pl, &pl->lower, sn * 8) != hipSuccess || gb_alloc(pl, &pl->upper, sn * 8) != hipSuccess ||
        gb_alloc(pl, &pl->index, sn * 4) != hipSuccess || gb_alloc(pl, &pl->npar, sn * 4) != hipSuccess ||
        gb_alloc(pl, &pl->created, sn * 4) != hipSuccess || gb_alloc(pl, &pl->expanded, sn) != hipSuccess ||
        gb_alloc(pl, &pl->visits, sn * 8) != hipSuccess || gb_alloc(pl, &pl->updates, sn * 8) != hipSuccess ||
        gb_alloc(pl, &pl->par, n * (size_t)pl->E * 4) != hipSuccess || gb_alloc(pl, &pl->queue, n * (size_t)pl->qcap * 4) != hipSuccess ||
        gb_alloc(pl, &pl->n_obs, n * 8) != hipSuccess || gb_alloc(pl, &pl->n_created, n * 4) != hipSuccess ||
        gb_alloc(pl, &pl->failed, n * 4) != hipSuccess || gb_alloc(pl, &pl->root_of, n * 4) != hipSuccess ||
        gb_alloc(pl, &pl->in_ptr, ((size_t)S + 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        mp_gbopd_free(pl);
        return fail(MP_ERR_ALLOC, "mp_gbopd_create: device allocation failed (%d planners x %d states, queue of %d entries each)",
                    n_planners, S, q);
    }
    // (stream order: the blocks may be recycled ones)
    if (hipMemsetAsync(pl->index, 0xff, sn * 4, st) != hipSuccess || hipMemsetAsync(pl->npar, 0, sn * 4, st) != hipSuccess ||
        hipMemsetAsync(pl->created, 0, sn * 4, st) != hipSuccess || hipMemsetAsync(pl->expanded, 0, sn, st) != hipSuccess ||
        hipMemsetAsync(pl->visits, 0, sn * 8, st) != hipSuccess || hipMemsetAsync(pl->updates, 0, sn * 8, st) != hipSuccess ||
        hipMemsetAsync(pl->lower, 0, sn * 8, st) != hipSuccess || hipMemsetAsync(pl->upper, 0, sn * 8, st) != hipSuccess ||
        hipMemsetAsync(pl->n_obs, 0, n * 8, st) != hipSuccess || hipMemsetAsync(pl->n_created, 0, n * 4, st) != hipSuccess ||
        hipMemsetAsync(pl->failed, 0, n * 4, st) != hipSuccess || hipMemsetAsync(pl->root_of, 0xff, n * 4, st) != hipSuccess ||
        hipMemcpyAsync(pl->in_ptr, pl->h_in_ptr.data(), ((size_t)S + 1) * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        mp_gbopd_free(pl);
        return fail(MP_ERR_HIP, "mp_gbopd_create: initialising the planners failed");
    }
    *out = pl;
    return MP_OK;
}

int mp_gbopd_plan(mp_ctx *ctx, mp_gbopd *pl, const int32_t *root_state, int32_t budget, double gamma, double value_max,
                  double accuracy, int32_t sampling_timeout, uint64_t *rng_state, int32_t *plans, int32_t *plan_len,
                  double *value_lower, double *value_upper, int64_t *env_steps, int64_t *updates, int32_t *status, int32_t mem)
{
    if (!ctx || !pl || !root_state || !rng_state) return fail(MP_ERR_ARG, "mp_gbopd_plan: NULL argument");
    int rmem;
    MP_TRY(wave_mem("mp_gbopd_plan", &mem, &rmem));
    if (pl->ctx != ctx) return fail(MP_ERR_ARG, "mp_gbopd_plan: planners belong to another context");
    if (pl->model->serial != pl->model_serial)
        return fail(MP_ERR_ARG, "mp_gbopd_plan: the model's tables or action sets changed under a kept graph (bounds, parents and "
                                "counters were built on the previous tables): free the planners and create new ones");
    if (sampling_timeout < 0) return fail(MP_ERR_ARG, "mp_gbopd_plan: sampling_timeout = %d", sampling_timeout);
    // (the reference never ends with a negative accuracy -- every pop appends its parents -- or with |gamma| >= 1, where the
    // bounds grow for ever: a device call must end)
    if (!(gamma > -1.0 && gamma < 1.0) || !(value_max == value_max) || !(accuracy >= 0.0))
        return fail(MP_ERR_ARG, "mp_gbopd_plan: need -1 < gamma < 1, accuracy >= 0 and a number for 1 / (1 - gamma)");
    const int n = pl->n, S = pl->S, A = pl->A;
    MP_TRY(wave_roots(ctx, "mp_gbopd_plan", root_state, n, S, mem));

    GbArgs a;
    a.n = n; a.S = S; a.A = A; a.K = budget > 0 ? budget / A : 0; // :120: budget // state.action_space.n
    a.timeout = sampling_timeout; a.qcap = pl->qcap; a.E = pl->E;
    a.max_pops = kGbMaxPops;
    if (const char *e = getenv("MP_GBOPD_MAX_POPS")) { // test knob: a smaller limit (never a larger one)
        const long v = atol(e);
        if (v >= 1 && v < kGbMaxPops) a.max_pops = v;
    }
    a.gamma = gamma; a.vmax = value_max; a.accuracy = accuracy;
    a.rec = pl->model->rec; a.in_ptr = pl->in_ptr;
    a.lower = pl->lower; a.upper = pl->upper; a.index = pl->index; a.npar = pl->npar; a.created = pl->created; a.par = pl->par;
    a.queue = pl->queue; a.n_created = pl->n_created; a.failed = pl->failed; a.root_of = pl->root_of; a.expanded = pl->expanded;
    a.visits = pl->visits; a.updates = pl->updates; a.n_obs = pl->n_obs;
    WaveIo io(mem, rmem, n, root_state, &a.root_state, rng_state, &a.rng);
    io.add(WS_IO3, plans, &a.plans, (size_t)sampling_timeout);
    io.add(WS_IO4, plan_len, &a.plan_len);
    io.add(WS_IO5, status, &a.status);
    io.add(WS_IO6, env_steps, &a.env_steps);
    io.add(WS_IO7, updates, &a.n_updates);
    io.add(WS_IO8, value_lower, &a.root_lower);
    io.add(WS_IO9, value_upper, &a.root_upper);
    MP_TRY(wave_stage(ctx, io));

    // both bounds in LDS while they are small (16 KiB: ten planners per CU); MP_GBOPD_LDS_BYTES moves the limit (0: never)
    size_t lds_limit = 16 * 1024;
    if (const char *e = getenv("MP_GBOPD_LDS_BYTES")) lds_limit = (size_t)atol(e);
    if (lds_limit > 64 * 1024) lds_limit = 64 * 1024;
    const size_t lds = (size_t)S * 16;
    const bool use_lds = lds <= lds_limit;
    MP_TRY(wave_launch(ctx, use_lds ? gbopd_kernel<true> : gbopd_kernel<false>, n, use_lds ? lds : 0, gbopd_form_name(use_lds), a));
    return wave_unstage(ctx, io);
}

int mp_gbopd_info(mp_gbopd *pl, int32_t *n_planners, int32_t *n_states, int32_t *n_actions, int32_t *queue_cap, int64_t *n_edges)
{
    if (!pl) return fail(MP_ERR_ARG, "mp_gbopd_info: planner is NULL");
    if (n_planners) *n_planners = pl->n;
    if (n_states) *n_states = pl->S;
    if (n_actions) *n_actions = pl->A;
    if (queue_cap) *queue_cap = pl->qcap;
    if (n_edges) *n_edges = pl->E;
    return MP_OK;
}

int mp_gbopd_export(mp_gbopd *pl, int32_t planner, int32_t cap, int32_t *n_nodes, int32_t *state, double *lower, double *upper,
                    uint8_t *expanded, int32_t *child, double *reward, int32_t *parent_ptr, int32_t *parent_idx,
                    int64_t *visits, int64_t *updates, int64_t *n_observations, int32_t *root)
{
    if (!pl || !n_nodes) return fail(MP_ERR_ARG, "mp_gbopd_export: NULL argument");
    if (planner < 0 || planner >= pl->n) return fail(MP_ERR_ARG, "mp_gbopd_export: planner %d out of range", planner);
    if (pl->model->serial != pl->model_serial)
        return fail(MP_ERR_ARG, "mp_gbopd_export: the model's tables or action sets changed under a kept graph: the children and "
                                "rewards of its nodes are no longer the model's");
    MP_HIP(hipSetDevice(pl->ctx->device));
    MP_HIP(hipStreamSynchronize(pl->ctx->stream));
    const size_t S = (size_t)pl->S, A = (size_t)pl->A, r = (size_t)planner;
    int32_t nc = 0, root_state = -1;
    int64_t nobs = 0;
    MP_HIP(hipMemcpy(&nc, pl->n_created + r, 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(&root_state, pl->root_of + r, 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(&nobs, pl->n_obs + r, 8, hipMemcpyDeviceToHost));
    if (nc < 0 || (size_t)nc > S) return fail(MP_ERR_ARG, "mp_gbopd_export: bad node count %d", nc);
    *n_nodes = nc;
    if (n_observations) *n_observations = nobs;
    if (cap < nc) return fail(MP_ERR_ARG, "mp_gbopd_export: capacity %d < %d nodes", cap, nc);
    std::vector<double> hl(S), hu(S);
    std::vector<int32_t> hidx(S), hnp(S), hcr(S), hpar((size_t)pl->E);
    std::vector<uint8_t> hex(S);
    MP_HIP(hipMemcpy(hl.data(), pl->lower + r * S, S * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hu.data(), pl->upper + r * S, S * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hidx.data(), pl->index + r * S, S * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hnp.data(), pl->npar + r * S, S * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hcr.data(), pl->created + r * S, S * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hex.data(), pl->expanded + r * S, S, hipMemcpyDeviceToHost));
    if (pl->E) MP_HIP(hipMemcpy(hpar.data(), pl->par + r * (size_t)pl->E, (size_t)pl->E * 4, hipMemcpyDeviceToHost));
    if (visits) MP_HIP(hipMemcpy(visits, pl->visits + r * S, S * 8, hipMemcpyDeviceToHost));
    if (updates) MP_HIP(hipMemcpy(updates, pl->updates + r * S, S * 8, hipMemcpyDeviceToHost));
    if (root) *root = root_state >= 0 && (size_t)root_state < S ? hidx[(size_t)root_state] : -1;
    int32_t np_total = 0;
    if (parent_ptr) parent_ptr[0] = 0;
    for (int32_t i = 0; i < nc; ++i) {
        const int32_t s = hcr[(size_t)i];
        if (s < 0 || (size_t)s >= S) return fail(MP_ERR_ARG, "mp_gbopd_export: node %d holds state %d", i, s);
        if (state) state[i] = s;
        if (lower) lower[i] = hl[(size_t)s];
        if (upper) upper[i] = hu[(size_t)s];
        if (expanded) expanded[i] = hex[(size_t)s];
        for (size_t a = 0; a < A; ++a) { // children and rewards per listed action (slot = listing order), -1 elsewhere
            const Rec &rc = pl->hrec[(size_t)s * A + a];
            const bool has = hex[(size_t)s] && (rc.flags & 4u);
            if (child) child[(size_t)i * A + a] = has ? hidx[(size_t)rc.next] : -1;
            if (reward) reward[(size_t)i * A + a] = has ? rc.reward : 0.0;
        }
        const int32_t base = pl->h_in_ptr[(size_t)s], room = pl->h_in_ptr[(size_t)s + 1] - base;
        const int32_t np = hnp[(size_t)s] < room ? hnp[(size_t)s] : room;
        for (int32_t j = 0; j < np; ++j) {
            const int32_t ps = hpar[(size_t)base + j];
            if (parent_idx) parent_idx[np_total] = ps >= 0 && (size_t)ps < S ? hidx[(size_t)ps] : -1;
            ++np_total;
        }
        if (parent_ptr) parent_ptr[i + 1] = np_total;
    }
    return MP_OK;
}

} // extern "C"
