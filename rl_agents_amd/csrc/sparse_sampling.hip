// sparse_sampling.hip -- Sparse Sampling (Kearns, Mansour, Ng), tree_search/sparse_sampling.py:11-96.
//
// Mapping: ONE ROOT PER WAVEFRONT (one 64-lane workgroup), the workgroups striding over the roots, as brue.hip.  A plan is the
// recursion DecisionNode.estimateV (:38-51) / ChanceNode.estimateQ (:71-88) to depth `horizon`, run here as an explicit stack
// of at most `horizon` frames:
//   * below a decision node at depth horizon - 1 nothing recurses, so the |A| C samples of all its listed actions are
//     consecutive in the stream: they are taken in ONE pass over the lanes, 64 at a time (sample t belongs to listed action
//     t / C), and the chance nodes are made action by action from the lanes that hold their samples.  This level holds the
//     bulk of a plan's samples; taking it action by action was 1.1x to 1.7x slower (profiles/sparse_sampling_last_level_ab.json)
//     and is gone.  Above that level the C samples of one chance node run on C lanes, 64 at a time;
//   * the draws.  Every sample draws np_random.randint(2**30) (:79): a
//     power-of-two range never rejects, so draw i is `half >> 2` of exactly one 32-bit half of the planner's stream, low half
//     first -- lane i jumps the generator ahead to its half-word (Pcg64::jump on the table of A^n, G_n), honouring a half that
//     was buffered at entry.  On a dense / sparse model the lane then seeds the clone's generator from its draw
//     (FiniteMDPEnv.seed: Generator(PCG64(SeedSequence(x))), seed_sequence.hpp), draws one double and finds the outcome in the
//     model's integer threshold row ceil(cdf * 2^53) (uct_stoch.hip builds them per model) by binary search;
//   * the distinct outcomes are listed in first-occurrence order with their counts (ChanceNode.get_child, :93-96, keyed by the
//     observation), across lanes and across chunks of 64: the lowest pending lane leads, the lanes that drew its outcome are
//     counted by one ballot;
//   * the backup `reward + gamma * sum(value * count) / C` (:87-88) is the serial chain of f64 operations in creation order
//     (Python's left-to-right sum from the int 0), `reward` the last sample's -- R(s, a) for every sample of a finite MDP;
//     DecisionNode.value is the first maximum over the listed actions (np.amax, :51).
// A wave reads back its frames only: per depth the decision node's running maximum and action cursor and the current chance
// node's outcome list (state, count; the children's node ids are consecutive).  The tree is a write-only log in global memory
// in creation order (the reference's order of dict insertion) whose only fix-up is the store of `value` when a node's
// recursion returns.  Two forms: the frames in LDS (ss_wave_lds) or in a global workspace (ss_wave_global).
// mp_ss_plan_models -- a batch model of deterministic tables, one MDP per root: a batch of agents that each hold their own
// environment -- runs the same kernel with the frames always in LDS (64 bytes a level) and the root's records read from the
// batch model (ss_each_global) or from a copy of the root's own table in LDS behind the frames (ss_each_lds); each_host.hpp
// picks.
// `done` is never read (:81); `gamma` enters as one multiplication per chance node: + * / on f64 and integer counts in the
// reference's order, results are bit-exact.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "each_host.hpp"
#include "opd_closing.hpp"
#include "pcg64.hpp"
#include "seed_sequence.hpp"
#include "wave.hpp"
#include "wave_host.hpp"

namespace mp {

constexpr size_t kSsKeepBytes = (size_t)1 << 30;  // trees of every root kept while they fit; also the most one tree may take
constexpr int kSsMaxHorizon = 16;
constexpr int kSsMaxC = 1024;
constexpr size_t kSsLdsDefault = 16 * 1024;       // frames in LDS up to here: ten waves a CU
constexpr size_t kSsLdsMax = 64 * 1024;           // what a workgroup may ask for
constexpr int kSsJumpEntries = 64;                // a chunk of 64 half-words is at most 33 generator steps

struct SsNode {
    double value;     // DecisionNode.value / ChanceNode.value (sparse_sampling.py:35,69): the int 0 is 0.0
    int32_t parent;
    int32_t key;      // chance node: the action; decision node: the observed state (-1 at the root)
    int32_t count;    // decision node: samples that led here (:83); chance node: 0
    int32_t depthc;   // depth | is_chance << 31
};
static_assert(sizeof(SsNode) == 24, "SsNode layout");

// what a wave keeps per depth: the decision node under evaluation and the chance node of its current action
struct SsFrame {
    double vmax, acc, reward;
    int32_t node, state, a, any; // decision node: id, state, action cursor, "a chance child returned"
    int32_t c, n_out, j, first;  // chance node: id, outcomes listed, the outcome whose subtree runs, id of outcome 0's node
};
static_assert(sizeof(SsFrame) == 56, "SsFrame layout");

struct SsArgs {
    int n_roots, A, H, C, mode, W, L, keep, grid, cap;
    double gamma;
    const Rec *rec;          // deterministic tables
    const uint64_t *thr;     // dense [S*A][S] / sparse [S*A][B]: ceil(cdf * 2^53)
    const int32_t *nxt;      // sparse: successors [S*A][B]
    const double *R;         // dense / sparse: reward [S*A]
    const uint8_t *avail;    // [S*A] actions the env lists, or nullptr: all
    const int32_t *root_state;
    const uint32_t *jump;    // [kSsJumpEntries][8] limbs of A^n and G_n
    uint64_t *rng;
    SsNode *nodes;           // [n_roots or 1][cap]
    double *rootq;           // [n_roots][A] values of the root's chance children
    char *frames;            // global form: [grid][H] frames
    int32_t *n_nodes_out;
    int32_t *plans, *status;
    double *root_value;
    int64_t *samples;
    int Sb;                  // one MDP per root: states per MDP of the batch model (a root's MDP starts at global state (s / Sb) * Sb)
};

__host__ __device__ inline size_t ss_frame_stride(int L) { return sizeof(SsFrame) + (size_t)L * sizeof(int2); }

// Nodes a tree can hold: D_0 = 1 decision node, chance_d = |A| D_d, D_(d+1) <= chance_d min(C, W).  -1: beyond int32.
inline int64_t ss_node_bound(int64_t A, int H, int64_t L)
{
    int64_t D = 1, total = 1;
    for (int d = 0; d < H; ++d) {
        const int64_t ch = A * D;
        D = ch * L;
        total += ch + D;
        if (total > INT32_MAX) return -1;
    }
    return total;
}

// strict increases of a threshold row = outcomes some 53-bit draw reaches
__global__ void ss_outdegree_kernel(const uint64_t *__restrict__ thr, long rows, int W, int32_t *__restrict__ out)
{
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const uint64_t *t = thr + row * W;
    uint64_t prev = 0;
    int n = 0;
    for (int j = 0; j < W; ++j) {
        const uint64_t v = t[j];
        n += v > prev ? 1 : 0;
        prev = v > prev ? v : prev;
    }
    atomicMax(out, n);
}

// Lane `lane` of a chunk of the planner's stream takes half-word `lane`: the half buffered at entry first, then the low and the
// high half of every output (one table-driven jump).  -> the outcome of one sample of row `sa`: np_random.randint(2**30) (:79)
// = half >> 2, the clone seeded with it and stepped once (:81).  A deterministic step consumes nothing else.
__device__ __forceinline__ int ss_sample(const SsArgs &p, const Pcg64 &gen, int lane, long sa)
{
    if (p.mode == MP_MODE_DETERMINISTIC) return p.rec[sa].next;
    const int idx = gen.has_uint32 ? lane - 1 : lane;              // which fresh half-word; -1: the buffered one
    uint32_t h = gen.uinteger;
    if (idx >= 0) {
        Pcg64 g = gen;
        const int k = (idx >> 1) + 1;
        uint32_t an[4], gn[4];
        for (int i = 0; i < 4; ++i) { an[i] = p.jump[k * 8 + i]; gn[i] = p.jump[k * 8 + 4 + i]; }
        g.jump(an, gn);
        const uint64_t o = g.output();
        h = (idx & 1) ? (uint32_t)(o >> 32) : (uint32_t)o;
    }
    const uint32_t x = h >> 2;                                     // (half * 2^30) >> 32
    uint64_t rec6[6];
    seed_sequence_record(&x, 1, rec6);                             // next_state.seed(x): the clone's generator
    Pcg64 eg;
    eg.s_hi = rec6[0]; eg.s_lo = rec6[1]; eg.inc_hi = rec6[2]; eg.inc_lo = rec6[3];
    eg.has_uint32 = 0; eg.uinteger = 0;
    const uint64_t kk = eg.next64() >> 11;                         // Generator.random() of the clone's step
    const uint64_t *trow = p.thr + sa * p.W;
    int lo = 0, hi = p.W;                                          // searchsorted(cdf, u, 'right') = #{j : thr_j <= k}
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (trow[mid] <= kk) lo = mid + 1; else hi = mid;
    }
    if (lo >= p.W) lo = p.W - 1;                                   // (u < 1 = cdf[-1]: not reached)
    return p.mode == MP_MODE_SPARSE ? p.nxt[sa * p.W + lo] : lo;
}

// the planner's generator after m 32-bit draws: the fresh halves are whole outputs, the last one maybe half used
__device__ __forceinline__ void ss_skip(const SsArgs &p, Pcg64 &gen, int m)
{
    const int fresh = gen.has_uint32 ? m - 1 : m;
    const int steps = (fresh + 1) >> 1;
    if (steps > 0) {
        uint32_t an[4], gn[4];
        for (int i = 0; i < 4; ++i) { an[i] = p.jump[steps * 8 + i]; gn[i] = p.jump[steps * 8 + 4 + i]; }
        gen.jump(an, gn);
        gen.uinteger = (uint32_t)(gen.output() >> 32);
    }
    gen.has_uint32 = (uint32_t)(fresh & 1);
}

// get_child(observation).count += 1 (:83) for the `pending` lanes' outcomes `sn`, in first-occurrence order: the lowest pending
// lane leads, one ballot counts the lanes that drew its outcome.  false: the list is full (cannot happen, L = min(C, W)).
__device__ __forceinline__ bool ss_list_add(int2 *list, int &n_out, int L, bool pending, int sn, int lane)
{
    unsigned long long pm = ballot64(pending);
    while (pm != 0ULL) {
        const int leader = __ffsll((long long)pm) - 1;
        const int v = __builtin_amdgcn_readlane(sn, leader);
        const unsigned long long mm = ballot64(pending && sn == v);
        const int cnt = __popcll(mm);
        int at = -1;
        for (int j0 = 0; j0 < n_out; j0 += 64) {
            const unsigned long long f = ballot64(j0 + lane < n_out && list[j0 + lane].x == v);
            if (f != 0ULL) { at = j0 + __ffsll((long long)f) - 1; break; }
        }
        if (at < 0) {
            if (n_out >= L) return false;
            if (lane == 0) list[n_out] = make_int2(v, cnt);
            ++n_out;
        } else if (lane == 0) {
            list[at].y += cnt;
        }
        __syncthreads();                                           // (one wavefront: the wait for lane 0's store)
        pending = pending && sn != v;
        pm &= ~mm;
    }
    return true;
}

// the n-th action the env lists in state s (columns are in listing order), A if there is none
__device__ __forceinline__ int ss_nth_listed(const uint8_t *avail, int s, int A, int n)
{
    if (!avail) return n < A ? n : A;
    int a = 0;
    for (; a < A; ++a)
        if (avail[(long)s * A + a] && n-- == 0) break;
    return a;
}

// EACH (mp_ss_plan_models: a batch model of deterministic tables, one MDP per root, the roots' states GLOBAL).  W = 1 on a table:
// an outcome list has one entry, a frame is 64 bytes and the frames always sit in LDS.  SS_EACH_GLOBAL reads the batch model's
// records as SS_WHOLE reads a single model's; SS_EACH_LDS copies the root's own Sb * |A| records into LDS behind the frames --
// once for consecutive roots of a workgroup that share an MDP -- and serves every model read of the root from there, the
// parallel reads of the one-pass last level included.  SS_WHOLE is the kernel of mp_ss_plan, as it was.
enum { SS_WHOLE = 0, SS_EACH_GLOBAL = 1, SS_EACH_LDS = 2 };
constexpr size_t kSsEachFrame = 64;                // sizeof(SsFrame) + one int2 list entry

template <bool LDSF, int EACH>
__global__ __launch_bounds__(64) void ss_kernel(SsArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char ss_smem[];
    constexpr bool each = EACH != SS_WHOLE;
    static_assert(!each || LDSF, "the frames of the one-MDP-per-root forms sit in LDS");
    const int lane = threadIdx.x, A = p.A, H = p.H, C = p.C;
    const size_t fstride = each ? kSsEachFrame : ss_frame_stride(p.L);
    char *const fbase = LDSF ? ss_smem : p.frames + (size_t)blockIdx.x * H * fstride;
    Rec *const lrec = reinterpret_cast<Rec *>(ss_smem + (size_t)H * kSsEachFrame);   // [Sb * A] SS_EACH_LDS: the root's table
    const double gamma = p.gamma;
    int mdp_base = 0, loaded = -1;                                 // SS_EACH_LDS: first global state of the root's MDP / of the MDP in LDS
    // record (s, a), s a GLOBAL state.  SS_EACH_LDS: at (s - mdp_base) * |A| + a of the copy; s is the root's state or the `next` of
    // one of this MDP's records, which the batch model's load-time validation keeps inside the MDP: s - mdp_base is in [0, Sb)
    auto rec_at = [&](long sa) -> const Rec & { return EACH == SS_EACH_LDS ? lrec[sa - (long)mdp_base * A] : p.rec[sa]; };
    for (int root = blockIdx.x; root < p.n_roots; root += p.grid) {
        const bool log = p.keep || root == 0;
        SsNode *const N = p.nodes + (p.keep ? (long)root * p.cap : 0);
        double *const rootq = p.rootq + (long)root * A;
        const int s_root = p.root_state[root];
        if constexpr (EACH == SS_EACH_LDS) {                       // (the previous root's reads ended at the barrier closing its iteration)
            mdp_base = s_root / p.Sb * p.Sb;
            if (mdp_base != loaded) {
                wave_lds_records(lrec, p.rec, mdp_base, A, p.Sb, lane);
                loaded = mdp_base;
                __syncthreads();
            }
        }
        if (log && lane == 0) {                                    // DecisionNode(parent=None), sparse_sampling.py:19
            SsNode r;
            r.value = 0.0; r.parent = -1; r.key = -1; r.count = 0; r.depthc = 0;
            N[0] = r;
        }
        Pcg64 gen;
        gen.load(p.rng + (long)root * 6);
        int n_nodes = 1, status = MP_OK;
        long samples = 0;
        // the frame in registers (wave-uniform); saved to frame d when the recursion goes down, loaded when it comes back
        int d = 0, node = 0, state = s_root, a = 0, any = 0;
        int c = -1, n_out = 0, j = 0, first = 0;
        double vmax = 0.0, acc = 0.0, reward = 0.0;
        for (;;) {
            SsFrame *const F = reinterpret_cast<SsFrame *>(fbase + d * fstride);
            int2 *const list = reinterpret_cast<int2 *>(F + 1);
            bool chance_done = false, descend = false;
            double q = 0.0;
            if (d + 1 == H) {
                // ---- a decision node at depth horizon - 1: nothing recurses below it, so the samples of ALL its listed actions
                // are consecutive in the stream -- sample t belongs to listed action t / C -- and are taken in one pass over
                // the lanes; the chance nodes are then made action by action, in order, from the lanes that hold their samples
                int k = 0;
                for (int b = 0; b < A; ++b) k += (!p.avail || p.avail[(long)state * A + b]) ? 1 : 0;
                const int total = k * C;
                bool bad = false;
                for (int base = 0; base < total && !bad; base += 64) {
                    const int m = total - base < 64 ? total - base : 64;
                    const int t = base + lane;
                    int sn = -1;
                    if (lane < m) {
                        const long sa = (long)state * A + ss_nth_listed(p.avail, state, A, t / C);
                        if constexpr (each) sn = rec_at(sa).next; else sn = ss_sample(p, gen, lane, sa);
                    }
                    ss_skip(p, gen, m);
                    for (int slot = base / C; slot * C < base + m && !bad; ++slot) {
                        a = ss_nth_listed(p.avail, state, A, slot);
                        if (slot * C >= base) {                    // get_child(action), :58-61
                            if (n_nodes + 1 > p.cap) { bad = true; break; }
                            c = n_nodes++;
                            n_out = 0;
                        }
                        bad = !ss_list_add(list, n_out, p.L, t >= slot * C && t < (slot + 1) * C && lane < m, sn, lane);
                        if (bad || (slot + 1) * C > base + m) continue;   // (the action's samples go on in the next chunk)
                        if (n_nodes + n_out > p.cap) { bad = true; break; }
                        const double r = each || p.mode == MP_MODE_DETERMINISTIC ? rec_at((long)state * A + a).reward : p.R[(long)state * A + a];
                        q = r + gamma * 0.0 / (double)C;           // the children hold the int 0 (:45-46, :87-88)
                        if (log) {
                            if (lane == 0) {
                                SsNode nd;
                                nd.value = q; nd.parent = node; nd.key = a; nd.count = 0; nd.depthc = d | (int)0x80000000;
                                N[c] = nd;
                            }
                            for (int i = lane; i < n_out; i += 64) {
                                const int2 e = list[i];
                                SsNode nd;
                                nd.value = 0.0; nd.parent = c; nd.key = e.x; nd.count = e.y; nd.depthc = d + 1;
                                N[n_nodes + i] = nd;
                            }
                        }
                        n_nodes += n_out;
                        if (d == 0 && lane == 0) rootq[a] = q;
                        if (!any || q > vmax) vmax = q;
                        any = 1;
                    }
                }
                samples += total;
                if (bad) { status = MP_ERR_ARG; break; }
                a = A;
            }
            // ---- DecisionNode.estimateV (:48-50): the next action the env lists
            while (a < A && p.avail && !p.avail[(long)state * A + a]) ++a;
            if (a < A) {
                if (n_nodes + 1 > p.cap) { status = MP_ERR_ARG; break; }   // (cannot happen: cap is the host's bound)
                c = n_nodes++;                                     // get_child(action), :58-61
                // ---- ChanceNode.estimateQ (:76-84): C samples, 64 at a time
                const long sa = (long)state * A + a;
                n_out = 0;
                if (each || p.mode == MP_MODE_DETERMINISTIC) {
                    const Rec rc = rec_at(sa);
                    reward = rc.reward;
                    if (lane == 0) list[0] = make_int2(rc.next, C);
                    n_out = 1;
                } else {
                    reward = p.R[sa];
                }
                bool full = false;
                for (int base = 0; base < C && !full; base += 64) {
                    const int m = C - base < 64 ? C - base : 64;
                    int sn = -1;
                    if (!each && p.mode != MP_MODE_DETERMINISTIC && lane < m) sn = ss_sample(p, gen, lane, sa);
                    ss_skip(p, gen, m);
                    full = !ss_list_add(list, n_out, p.L, sn >= 0, sn, lane);
                }
                __syncthreads();
                samples += C;
                if (full || n_nodes + n_out > p.cap) { status = MP_ERR_ARG; break; }
                first = n_nodes;
                n_nodes += n_out;
                if (log) {
                    if (lane == 0) {                               // ChanceNode(parent), :64-69
                        SsNode nd;
                        nd.value = 0.0; nd.parent = node; nd.key = a; nd.count = 0; nd.depthc = d | (int)0x80000000;
                        N[c] = nd;
                    }
                    for (int i = lane; i < n_out; i += 64) {       // DecisionNode(parent), :32-36, in creation order
                        const int2 e = list[i];
                        SsNode nd;
                        nd.value = 0.0; nd.parent = c; nd.key = e.x; nd.count = e.y; nd.depthc = d + 1;
                        N[first + i] = nd;
                    }
                }
                acc = 0.0; j = 0;                                  // (d + 1 < H: the last level is taken above)
                descend = true;
            } else {
                // ---- every listed action is done: value = np.amax(children values), :51
                if (log && lane == 0) N[node].value = vmax;
                if (d == 0) break;
                const double v = vmax;
                --d;
                SsFrame *const G = reinterpret_cast<SsFrame *>(fbase + d * fstride);
                const SsFrame f = *G;
                node = f.node; state = f.state; a = f.a; any = f.any; vmax = f.vmax;
                c = f.c; n_out = f.n_out; j = f.j; first = f.first; acc = f.acc; reward = f.reward;
                const int2 e = reinterpret_cast<const int2 *>(G + 1)[j];
                acc = acc + v * (double)e.y;                       // sum(value * count), left to right from the int 0, :87
                ++j;
                if (j < n_out) {
                    descend = true;
                } else {
                    q = reward + gamma * acc / (double)C;          // :87-88
                    chance_done = true;
                }
            }
            if (chance_done) {
                if (log && lane == 0) N[c].value = q;
                if (d == 0 && lane == 0) rootq[a] = q;
                if (!any || q > vmax) vmax = q;                    // np.amax: the first maximum
                any = 1;
                ++a;
            } else if (descend) {
                // estimateV of outcome j (:85-86): this frame waits
                SsFrame *const G = reinterpret_cast<SsFrame *>(fbase + d * fstride);
                const int2 e = reinterpret_cast<const int2 *>(G + 1)[j];
                if (lane == 0) {
                    SsFrame f;
                    f.vmax = vmax; f.acc = acc; f.reward = reward; f.node = node; f.state = state; f.a = a; f.any = any;
                    f.c = c; f.n_out = n_out; f.j = j; f.first = first;
                    *G = f;
                }
                __syncthreads();
                node = first + j; state = e.x; a = 0; any = 0; vmax = 0.0;
                ++d;
            }
        }
        __syncthreads();
        // ---- get_plan (:26-28): root.selection_rule() (:53-56) = random_argmax over the chance children in listing order
        int plan = -1;
        double value = 0.0;
        if (status == MP_OK && any) {
            const int s0 = s_root;
            const double m = vmax;
            plan = draw_tie_chunks(A, [&](int b) { return (!p.avail || p.avail[(long)s0 * A + b]) && rootq[b] == m; }, gen);
            value = rootq[plan];
        }
        if (lane == 0) {
            gen.store(p.rng + (long)root * 6);
            if (p.plans) p.plans[root] = plan;
            if (p.status) p.status[root] = status;
            if (p.samples) p.samples[root] = samples;
            if (p.root_value) p.root_value[root] = value;
            p.n_nodes_out[root] = n_nodes;
        }
        __syncthreads();
    }
}

// the widest outcome list a chance node of `model` can have: 1 for tables, B for sparse rows, the fullest row's reachable
// outcomes for dense ones (counted once per model on the device from the thresholds)
static int ss_outdegree(mp_ctx *ctx, mp_model *model, int *W)
{
    if (model->mode == MP_MODE_DETERMINISTIC) { *W = 1; return MP_OK; }
    if (model->mode == MP_MODE_SPARSE) { *W = model->B; return MP_OK; }
    if (model->ss_w > 0 && model->ss_w_serial == model->serial) { *W = model->ss_w; return MP_OK; }
    int32_t *d = nullptr;
    MP_TRY(ws_get(ctx, WS_IO9, (size_t)1, &d));                     // (a slot no tree export reads: the call may still be refused)
    MP_HIP(hipMemsetAsync(d, 0, sizeof(int32_t), ctx->stream));
    const long rows = (long)model->S * model->A;
    hipLaunchKernelGGL(ss_outdegree_kernel, dim3((unsigned)((rows + 127) / 128)), dim3(128), 0, ctx->stream, model->thr, rows, model->S, d);
    MP_HIP(hipGetLastError());
    int32_t w = 0;
    MP_HIP(hipMemcpyAsync(&w, d, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MP_HIP(hipStreamSynchronize(ctx->stream));
    if (w < 1) w = 1;
    model->ss_w = w; model->ss_w_serial = model->serial;
    *W = w;
    return MP_OK;
}

// the PCG64 jump-ahead table of uct.hip (limbs of A^n and G_n, n < ctx->jump_entries) resident in WS_JUMP
static int ss_jump_table(mp_ctx *ctx, const uint32_t **out)
{
    if (ctx->jump_entries < kSsJumpEntries) {
        typedef unsigned __int128 u128;
        const u128 mult = ((u128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL;
        ctx->jump_host.emplace_back((size_t)kSsJumpEntries * 8, 0u); // (kept: the upload is asynchronous)
        std::vector<uint32_t> &tab = ctx->jump_host.back();
        u128 an = 1, gn = 0;
        for (int n = 0; n < kSsJumpEntries; ++n) {
            for (int i = 0; i < 4; ++i) { tab[(size_t)n * 8 + i] = (uint32_t)(an >> (32 * i)); tab[(size_t)n * 8 + 4 + i] = (uint32_t)(gn >> (32 * i)); }
            gn = gn * mult + 1;
            an = an * mult;
        }
        uint32_t *dj = nullptr;
        ctx->jump_entries = 0;
        MP_TRY(ws_get(ctx, WS_JUMP, tab.size(), &dj));
        MP_HIP(hipMemcpyAsync(dj, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        ctx->jump_entries = kSsJumpEntries;
    }
    *out = static_cast<const uint32_t *>(ctx->ws[WS_JUMP].p);
    return MP_OK;
}

// frames in LDS?  MP_SS_FRAMES=lds|global forces either form where it is legal (read at each call)
static bool ss_use_lds(size_t frame_bytes)
{
    bool use = frame_bytes <= kSsLdsDefault;
    if (const char *e = getenv("MP_SS_FRAMES")) {
        if (!strcmp(e, "global")) use = false;
        else if (!strcmp(e, "lds")) use = frame_bytes <= kSsLdsMax;
    }
    return use;
}

} // namespace mp

using namespace mp;

extern "C" {

int mp_ss_geometry(int32_t n_actions, int32_t horizon, int32_t C, int32_t W, int64_t *out)
{
    if (!out) return fail(MP_ERR_ARG, "mp_ss_geometry: NULL argument");
    if (n_actions < 1 || horizon < 1 || horizon > kSsMaxHorizon || C < 1 || C > kSsMaxC || W < 1)
        return fail(MP_ERR_ARG, "mp_ss_geometry: need 1 <= horizon <= %d, 1 <= C <= %d, |A| >= 1 and W >= 1", kSsMaxHorizon, kSsMaxC);
    const int L = C < W ? C : W;
    out[0] = L;
    out[1] = (int64_t)(horizon * ss_frame_stride(L));
    out[2] = ss_node_bound(n_actions, horizon, L);
    out[3] = (int64_t)kSsLdsDefault;
    out[4] = ss_use_lds((size_t)out[1]) ? 1 : 0;
    return MP_OK;
}

const char *mp_ss_form_names(void)
{
    static const std::string names = std::string(ss_form_name(true).s) + "\n" + ss_form_name(false).s + "\n";
    return names.c_str();
}

const char *mp_ss_each_form_names(void)
{
    static const std::string names = ss_each_form_names();
    return names.c_str();
}

extern "C++" {
namespace {
// mp_ss_plan (each = false: `root_state` holds states of the one model) and mp_ss_plan_models (each = true: a batch model of
// deterministic tables; it holds the GLOBAL states globalize_roots_arg made of the (model_index, local state) pairs, the frames
// sit in LDS and the form is each_form's)
int ss_plan_impl(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t horizon, int32_t C, double gamma,
                 uint64_t *rng_state, int32_t *plans, double *root_value, int64_t *samples, int32_t *status, int32_t mem, bool each)
{
    const char *const who = each ? "mp_ss_plan_models" : "mp_ss_plan";
    if (!ctx || !model || !root_state || !rng_state) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    int rmem;
    MP_TRY(wave_mem(who, &mem, &rmem));
    MP_TRY(wave_mdp_check(who, model, each));
    const int A = model->A;
    if (n_roots < 1 || A < 1) return fail(MP_ERR_ARG, "%s: bad sizes", who);
    // (horizon 0: the root gets no child and the reference's selection raises; C 0: its backup reads a reward no sample set)
    if (horizon < 1 || horizon > kSsMaxHorizon)
        return fail(MP_ERR_ARG, "%s: horizon %d: the frames serve 1 <= horizon <= %d", who, horizon, kSsMaxHorizon);
    if (C < 1 || C > kSsMaxC) return fail(MP_ERR_ARG, "%s: C %d: the frames serve 1 <= C <= %d samples", who, C, kSsMaxC);
    MP_TRY(wave_roots(ctx, who, root_state, n_roots, model->S, mem));
    SsArgs a;
    MP_TRY(wave_mdp(ctx, who, model, &a));
    int W = 1;
    MP_TRY(ss_outdegree(ctx, model, &W));

    a.L = C < W ? C : W;
    const int64_t bound = ss_node_bound(A, horizon, a.L);
    if (bound < 0)
        return fail(MP_ERR_ARG, "%s: a tree of %d actions, horizon %d and %d outcomes a sample set does not fit int32 node indices", who,
                    A, horizon, a.L);
    const size_t per_tree = (size_t)bound * sizeof(SsNode);
    if (per_tree > kSsKeepBytes) return fail(MP_ERR_ARG, "%s: a tree of up to %ld nodes does not fit the workspace", who, (long)bound);
    size_t keep_bytes = kSsKeepBytes;
    if (const char *e = getenv("MP_SS_KEEP_BYTES")) { // test knob: a smaller workspace (never a larger one)
        const long long v = atoll(e);
        if (v >= 0 && (size_t)v < keep_bytes) keep_bytes = (size_t)v;
    }
    // (the global form is the launch mp_ss_plan always made: CUs * 32 wavefronts at most)
    const int cus = ctx->prop.multiProcessorCount;
    a.Sb = model->Sb > 0 ? model->Sb : model->S;
    const EachForm form = each ? each_form(EACH_SS, a.Sb, A, horizon, n_roots, cus) : each_form_global(EACH_SS, horizon, n_roots, cus);
    a.grid = form.grid;
    a.n_roots = n_roots; a.A = A; a.H = horizon; a.C = C; a.cap = (int)bound; a.gamma = gamma;
    a.avail = model->masked ? model->avail : nullptr;
    MP_TRY(ss_jump_table(ctx, &a.jump));
    const size_t frame_bytes = (size_t)horizon * ss_frame_stride(a.L);
    const bool use_lds = each || ss_use_lds(frame_bytes);              // (one MDP per root: W = 1, at most 1 KiB of frames)
    a.frames = nullptr;
    if (!use_lds) MP_TRY(ws_get(ctx, WS_TREE2, (size_t)a.grid * frame_bytes, &a.frames));
    MP_TRY(ws_get(ctx, WS_TREE1, (size_t)n_roots * A, &a.rootq)); // (not a per-slot array here)
    MP_TRY(wave_tree(ctx, 7, n_roots, A, bound, 0, keep_bytes, 1, 0, &a.nodes, (double **)nullptr, &a.n_nodes_out, &a.keep));
    WaveIo io(mem, rmem, n_roots, root_state, &a.root_state, rng_state, &a.rng);
    io.add(WS_IO3, plans, &a.plans);
    io.add(WS_IO5, root_value, &a.root_value);
    io.add(WS_IO7, status, &a.status);
    io.add(WS_IO8, samples, &a.samples);
    MP_TRY(wave_stage(ctx, io));
    if (each)
        MP_TRY(wave_launch(ctx, form.lds ? ss_kernel<true, SS_EACH_LDS> : ss_kernel<true, SS_EACH_GLOBAL>, a.grid, form.lds_bytes(),
                           ss_each_form_name(form.lds), a));
    else
        MP_TRY(wave_launch(ctx, use_lds ? ss_kernel<true, SS_WHOLE> : ss_kernel<false, SS_WHOLE>, a.grid, use_lds ? frame_bytes : 0,
                           ss_form_name(use_lds), a));
    return wave_unstage(ctx, io);
}
} // namespace
} // extern "C++"

int mp_ss_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t horizon, int32_t C, double gamma,
               uint64_t *rng_state, int32_t *plans, double *root_value, int64_t *samples, int32_t *status, int32_t mem)
{
    return ss_plan_impl(ctx, model, n_roots, root_state, horizon, C, gamma, rng_state, plans, root_value, samples, status, mem, false);
}

int mp_ss_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                      int32_t horizon, int32_t C, double gamma, uint64_t *rng_state, int32_t *plans, double *root_value,
                      int64_t *samples, int32_t *status, int32_t mem)
{
    if (!mem_valid(mem)) return fail(MP_ERR_ARG, "mp_ss_plan_models: unknown mem flags %d", mem);
    std::vector<int32_t> tmp;
    const int32_t *global = nullptr;
    MP_TRY(globalize_roots_arg(ctx, model, n_roots, model_index, root_state, mem, tmp, &global));
    return ss_plan_impl(ctx, model, n_roots, global, horizon, C, gamma, rng_state, plans, root_value, samples, status, mem, true);
}

int mp_ss_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *key, uint8_t *is_chance,
                      int32_t *depth, int64_t *count, double *value)
{
    int32_t slot, n;
    MP_TRY(wave_export_begin(ctx, 7, "mp_ss_tree_export", "mp_ss_plan", root, &slot, &n));
    if (n_nodes) *n_nodes = n;                                     // (before the refusal: the caller learns the capacity it needs)
    if (n > cap) return fail(MP_ERR_ARG, "mp_ss_tree_export: capacity %d < %d nodes", cap, n);
    std::vector<SsNode> na((size_t)n);
    MP_TRY(wave_pull(ctx, WS_TREE0, slot, n, sizeof(SsNode), na.data()));
    for (int i = 0; i < n; ++i) {
        if (parent) parent[i] = na[i].parent;
        if (key) key[i] = na[i].key;
        if (is_chance) is_chance[i] = na[i].depthc < 0 ? 1 : 0;
        if (depth) depth[i] = na[i].depthc & 0x7fffffff;
        if (count) count[i] = na[i].count;
        if (value) value[i] = na[i].value;
    }
    return MP_OK;
}

} // extern "C"
