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

#include <new>
#include <vector>

#include "common.hpp"
#include "graph_shared.hpp"
#include "opd_closing.hpp"
#include "pcg64.hpp"
#include "wave.hpp"

struct mp_gbopd : mp::GraphHandle {
    int64_t *updates = nullptr;
    std::vector<mp::Rec> hrec;  // host copy of the model's records (in-degrees at creation, children / rewards of the export)
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
    int64_t *env_steps, *pops;
};

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
        if (l0) graph_refuse(r, status, p.plan_len, p.status, p.root_lower, p.root_upper, p.env_steps, p.pops);
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
    if (LDSV) graph_stage_in(p.lower, p.upper, sb, created, n_created, lower, upper, lane); // the bounds of the nodes that exist
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
                if (pops_total + pops >= p.max_pops) { status = MP_ERR_GBOPD_DIVERGED; break; } // (see kGraphMaxPops: the front stays unpopped)
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
    if (LDSV) graph_write_back(p.lower, p.upper, sb, created, n_created, lower, upper, lane);
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
        if (p.pops) p.pops[r] = pops_total;
    }
}

} // namespace mp

using namespace mp;

extern "C" {

int mp_gbopd_free(mp_gbopd *pl) { return graph_free(pl); }

int mp_gbopd_create(mp_ctx *ctx, mp_model *model, int32_t n_planners, int32_t queue_cap, mp_gbopd **out)
{
    const char *const who = "mp_gbopd_create";
    if (!ctx || !model || !out) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    if (model->mode != MP_MODE_DETERMINISTIC || !model->rec)
        return fail(MP_ERR_MODE, "%s: GBOP-D needs a deterministic table model (mode %d)", who, model->mode);
    if (model->M != 1 || model->NB != 1) return fail(MP_ERR_MODE, "%s: one whole model expected (no joint or batch model)", who);
    if (n_planners < 1 || model->S < 1 || model->A < 1) return fail(MP_ERR_ARG, "%s: n_planners = %d", who, n_planners);
    MP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    mp_gbopd *pl = new (std::nothrow) mp_gbopd;
    if (!pl) return fail(MP_ERR_ALLOC, "%s: out of memory", who);
    pl->ctx = ctx; pl->model = model; pl->model_serial = model->serial; pl->n = n_planners; pl->S = model->S; pl->A = model->A;
    const int S = pl->S, A = pl->A;
    pl->qcap = graph_queue_capacity(queue_cap, "MP_GBOPD_QUEUE", n_planners);
    // the model's records on the host; a listed (s, a) leads to its one next state
    pl->hrec.resize((size_t)S * A);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(pl->hrec.data(), model->rec, (size_t)S * A * sizeof(Rec), hipMemcpyDeviceToHost) != hipSuccess) {
        delete pl;
        return fail(MP_ERR_HIP, "%s: reading the model's records failed", who);
    }
    const int counted = graph_count_parents(pl, who, [&](int s, int a, auto visit) {
        const Rec &rc = pl->hrec[(size_t)s * A + a];
        return rc.flags & 4u ? visit(rc.next) : (int)MP_OK;
    });
    if (counted != MP_OK) {
        delete pl;
        return counted;
    }
    const size_t sn = (size_t)S * pl->n;
    const int q = pl->qcap;
    int made = graph_create_shared(pl);
    if (made == MP_OK && graph_alloc(pl, &pl->updates, sn * 8) != hipSuccess) made = MP_ERR_ALLOC;
    if (made == MP_OK && (hipMemsetAsync(pl->updates, 0, sn * 8, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) made = MP_ERR_HIP;
    if (made != MP_OK) {
        (void)hipGetLastError();
        mp_gbopd_free(pl);
        if (made == MP_ERR_HIP) return fail(MP_ERR_HIP, "%s: initialising the planners failed", who);
        return fail(MP_ERR_ALLOC, "%s: device allocation failed (%d planners x %d states, queue of %d entries each)", who, n_planners, S, q);
    }
    *out = pl;
    return MP_OK;
}

int mp_gbopd_plan(mp_ctx *ctx, mp_gbopd *pl, const int32_t *root_state, int32_t budget, double gamma, double value_max,
                  double accuracy, int32_t sampling_timeout, uint64_t *rng_state, int32_t *plans, int32_t *plan_len,
                  double *value_lower, double *value_upper, int64_t *env_steps, int64_t *updates, int32_t *status, int32_t mem)
{
    const char *const who = "mp_gbopd_plan";
    if (!ctx || !pl || !root_state || !rng_state) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    int rmem;
    MP_TRY(wave_mem(who, &mem, &rmem));
    MP_TRY(graph_check_handle(ctx, pl, who, "bounds, parents and counters"));
    if (sampling_timeout < 0) return fail(MP_ERR_ARG, "%s: sampling_timeout = %d", who, sampling_timeout);
    MP_TRY(graph_check_numbers(who, gamma, value_max, accuracy));
    const int n = pl->n, S = pl->S, A = pl->A;
    MP_TRY(wave_roots(ctx, who, root_state, n, S, mem));

    GbArgs a;
    graph_args(pl, "MP_GBOPD_MAX_POPS", gamma, value_max, accuracy, &a);
    a.K = budget > 0 ? budget / A : 0; // :120: budget // state.action_space.n
    a.timeout = sampling_timeout;
    a.rec = pl->model->rec; a.updates = pl->updates;
    WaveIo io(mem, rmem, n, root_state, &a.root_state, rng_state, &a.rng);
    io.add(WS_IO3, plans, &a.plans, (size_t)sampling_timeout);
    graph_results_io(io, plan_len, status, env_steps, updates, value_lower, value_upper, &a);
    MP_TRY(wave_stage(ctx, io));

    // both bounds in LDS while they are small; MP_GBOPD_LDS_BYTES moves the limit
    const bool use_lds = graph_use_lds("MP_GBOPD_LDS_BYTES", S);
    MP_TRY(wave_launch(ctx, use_lds ? gbopd_kernel<true> : gbopd_kernel<false>, n, use_lds ? (size_t)S * 16 : 0, gbopd_form_name(use_lds), a));
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
    const char *const who = "mp_gbopd_export";
    GraphExport x;
    MP_TRY(graph_export_begin(pl, who, "children and rewards", planner, cap, n_nodes, visits, n_observations, root, &x));
    const size_t S = (size_t)pl->S, A = (size_t)pl->A;
    if (updates) MP_HIP(hipMemcpy(updates, pl->updates + (size_t)planner * S, S * 8, hipMemcpyDeviceToHost));
    int32_t np_total = 0;
    if (parent_ptr) parent_ptr[0] = 0;
    for (int32_t i = 0; i < x.n_nodes; ++i) {
        const int32_t s = x.created[(size_t)i];
        if (s < 0 || (size_t)s >= S) return fail(MP_ERR_ARG, "%s: node %d holds state %d", who, i, s);
        if (state) state[i] = s;
        if (lower) lower[i] = x.lower[(size_t)s];
        if (upper) upper[i] = x.upper[(size_t)s];
        if (expanded) expanded[i] = x.expanded[(size_t)s];
        for (size_t a = 0; a < A; ++a) { // children and rewards per listed action (slot = listing order), -1 elsewhere
            const Rec &rc = pl->hrec[(size_t)s * A + a];
            const bool has = x.expanded[(size_t)s] && (rc.flags & 4u);
            if (child) child[(size_t)i * A + a] = has ? x.index[(size_t)rc.next] : -1;
            if (reward) reward[(size_t)i * A + a] = has ? rc.reward : 0.0;
        }
        graph_export_parents(pl, x, i, s, parent_ptr, parent_idx, &np_total);
    }
    return MP_OK;
}

} // extern "C"
