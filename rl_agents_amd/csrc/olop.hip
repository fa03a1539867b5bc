// olop.hip -- Open-Loop Optimistic Planning, OLOP / KL-OLOP (tree_search/olop.py, utils.py:89-203).
//
// Mapping: ONE ROOT PER WAVEFRONT (one 64-lane workgroup), the workgroups striding over the roots.  An OLOP plan is M episodes
// of exactly L model steps down a tree of action sequences that grows only where it is walked (olop.py:64-92):
//   * the walk is the serial chain: one model step per depth, every lane holding the same (wave-uniform) state;
//   * the lanes cover a node's children -- their creation at an expansion (one 16-byte model gather each, listing order by a
//     ballot prefix count), the selection argmax (Python max with `>`, olop.py:84) and the backup's np.amax (olop.py:188, NaN
//     propagating) -- 64 at a time when |A| > 64;
//   * the L bounds of an episode's path are independent (each node appears once on the path and only the backup reads them),
//     so the lanes cover the L path nodes and run their Newton iterations (utils.py:123-203) at the same time, after the walk.
// Nodes live in a global workspace, children contiguous in creation order (the reference's order of dict insertion): at most
// 1 + M * L * |A| nodes per tree, a tree per root or per workgroup (wave_host.hpp: wave_tree).  Everything that is not a basic
// IEEE operation -- the initial upper bounds (Python **), the thresholds (eval of the config string, np.log) -- comes from
// host tables.  The Newton step's log is the device's (parity of the bounds is 1e-12, not bit-exact).
// olop_kernel plans on deterministic tables (mp_olop_plan, mp_olop_plan_models); olop_stoch_kernel, below it, on dense and sparse
// models (mp_olop_plan_stochastic), where the state is the episode's and the clone's own generator samples every step.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "each_host.hpp"
#include "kl_bound.hpp"
#include "pcg64.hpp"
#include "seed_sequence.hpp"
#include "wave.hpp"
#include "wave_host.hpp"

namespace mp {

constexpr size_t kOlopKeepBytes = (size_t)1 << 30; // trees of every root kept while they fit

struct OlopNode {
    double cum, mu;                  // cumulative_reward, mu_ucb (olop.py:102-108)
    int32_t count, state, parent, first_child;
    int32_t n_children, action, depth, done;
};
static_assert(sizeof(OlopNode) == 48, "OlopNode layout");

struct OlopArgs {
    int n_roots, A, M, L, cap, done_on_next, kl, cont, keep, grid, max_plan_len;
    double gamma;
    const Rec *rec;
    const int32_t *root_state;
    const double *thr;   // [M]     threshold of episode e
    const double *vinit; // [L + 1] (1 - gamma ** (L + 1 - d)) / (1 - gamma)
    uint64_t *rng;
    OlopNode *nodes;     // [slots][cap]
    double *vu;          // [slots][cap] value_upper
    int32_t *n_nodes_out;
    int32_t *plans, *plan_len, *status;
    double *root_value;
    int64_t *env_steps;
    int Sb;              // LDS_MODEL: states per MDP of the batch model (a root's MDP starts at global state (s / Sb) * Sb)
};

// bernoulli_kl and kl_upper_bound (utils.py:89-203) are in kl_bound.hpp, which gape.hip includes too

__device__ __forceinline__ unsigned long long olop_ballot(bool p) { return __ballot(p); }

// Python max over children [0, k) in order with `>` (olop.py:84, and the tie-break of selection_rule :126-130 when `in_set`
// restricts it): the first element stays unless something is strictly greater, so a NaN first element wins and later NaNs
// never do.  Returns the index (wave-uniform).
__device__ int olop_first_max(const double *V, const OlopNode *C, int k, int lane, int count_eq)
{
    // first element of the set
    int first = 0x7fffffff;
    for (int i0 = 0; i0 < k && first == 0x7fffffff; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < k && (count_eq < 0 || C[i].count == count_eq);
        const unsigned long long bal = olop_ballot(in);
        if (bal) first = i0 + __ffsll((long long)bal) - 1;
    }
    if (isnan(V[first])) return first;
    double bv = 0.0;
    int bi = 0x7fffffff;
    bool have = false;
    for (int i = lane; i < k; i += 64) {
        if (count_eq >= 0 && C[i].count != count_eq) continue;
        const double v = V[i];
        if (!isnan(v) && (!have || v > bv)) { bv = v; bi = i; have = true; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        const int oh = __shfl_xor((int)have, off);
        if (oh && (!have || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; have = true; }
    }
    return bi;
}

// np.amax over children [0, k): NaN if any is NaN (olop.py:188)
__device__ double olop_amax(const double *V, int k, int lane)
{
    double m = -INFINITY;
    bool nan_seen = false;
    for (int i = lane; i < k; i += 64) {
        const double v = V[i];
        if (isnan(v)) nan_seen = true;
        else if (v > m) m = v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    return olop_ballot(nan_seen) ? (double)NAN : m;
}

// LDS_MODEL (mp_olop_plan_models, one MDP per root): the root's own Sb * |A| records sit in LDS behind path[], copied before
// its first episode, and every model read -- the expansion's gather, the step -- is served from there.  The `false`
// instantiation is the kernel of mp_olop_plan as it was: everything the LDS form adds sits under `if constexpr`, and the two
// compile to the same instructions (profiles/each_kernel_resources.txt).
template <bool LDS_MODEL>
__global__ __launch_bounds__(64) void olop_kernel(OlopArgs p)
{
    extern __shared__ int32_t path[]; // [L + 1] node ids of the episode's walk
    const int lane = threadIdx.x, A = p.A, L = p.L;
    Rec *lrec = nullptr;              // [Sb * A] LDS_MODEL: the root's table, 16-byte aligned behind path[]
    if constexpr (LDS_MODEL)
        lrec = static_cast<Rec *>(__builtin_assume_aligned(path + ((L + 1 + 3) & ~3), 16));
    const uint32_t done_bit = p.done_on_next ? 2u : 1u;
    const double mu0 = p.kl ? 1.0 : (double)INFINITY; // olop.py:105-108
    for (int root = blockIdx.x; root < p.n_roots; root += p.grid) {
        const long slot = p.keep ? root : (root == 0 ? p.grid : blockIdx.x);
        OlopNode *N = p.nodes + slot * p.cap;
        double *V = p.vu + slot * p.cap;
        // LDS_MODEL: the root's table into LDS (the previous root's reads ended at the barrier that closes its iteration; this
        // root's begin after the one below)
        int s_root = 0, base = 0;
        if constexpr (LDS_MODEL) {
            s_root = p.root_state[root];
            base = s_root / p.Sb * p.Sb;
            wave_lds_records(lrec, p.rec, base, A, p.Sb, lane);
        }
        if (lane == 0) {
            OlopNode r;
            r.cum = 0.0; r.mu = mu0; r.count = 0; r.state = LDS_MODEL ? s_root : p.root_state[root]; r.parent = -1; r.first_child = -1;
            r.n_children = 0; r.action = -1; r.depth = 0; r.done = 0;
            N[0] = r;
            V[0] = p.vinit[0];
        }
        __syncthreads();
        Pcg64 gen;
        gen.load(p.rng + (long)root * 6);
        int n_nodes = 1, status = MP_OK;
        long steps = 0;
        for (int e = 0; e < p.M && status == MP_OK; ++e) {
            gen.below(1u << 30); // state.seed(self.np_random.randint(2**30)), olop.py:73
            int node = 0;
            if (lane == 0) path[0] = 0;
            for (int h = 0; h < L; ++h) {
                const OlopNode nd = N[node];
                int fc = nd.first_child, k = nd.n_children, j, act;
                if (k == 0) {
                    // OLOPNode.expand (olop.py:165-180): the available actions in listing order
                    const Rec *row = LDS_MODEL ? lrec + (nd.state - base) * A : p.rec + (long)nd.state * A;
                    int rank0 = -1, pos0 = 0;
                    fc = n_nodes;
                    for (int a0 = 0; a0 < A; a0 += 64) {
                        const int a = a0 + lane;
                        Rec rc;
                        bool av = false;
                        if (a < A) { rc = row[a]; av = (rc.flags & 4u) != 0; }
                        const unsigned long long bal = olop_ballot(av);
                        const int pos = pos0 + __popcll(bal & ((1ull << lane) - 1ull));
                        if (av) {
                            OlopNode c;
                            c.cum = 0.0; c.mu = mu0; c.count = 0; c.state = rc.next; c.parent = node; c.first_child = -1;
                            c.n_children = 0; c.action = a; c.depth = nd.depth + 1; c.done = 0;
                            N[fc + pos] = c;
                            V[fc + pos] = p.vinit[nd.depth + 1];
                        }
                        if (p.cont >= a0 && p.cont < a0 + 64 && ((bal >> (p.cont - a0)) & 1ull))
                            rank0 = pos0 + __popcll(bal & ((1ull << (p.cont - a0)) - 1ull));
                        pos0 += __popcll(bal);
                    }
                    k = pos0;
                    if (lane == 0) { N[node].first_child = fc; N[node].n_children = k; }
                    n_nodes += k;
                    __syncthreads();
                    if (p.cont < 0) { // np_random.choice(list(children))
                        j = (int)gen.below((uint32_t)k);
                        act = N[fc + j].action;
                    } else { // action 0 (in the env's numbering): KeyError when it is not a child
                        j = rank0;
                        act = p.cont;
                    }
                } else {
                    j = olop_first_max(V + fc, N + fc, k, lane, -1);
                    act = N[fc + j].action;
                }
                // the model step (every step is taken: the reference does not stop at done)
                const Rec rc = LDS_MODEL ? lrec[(nd.state - base) * A + act] : p.rec[(long)nd.state * A + act];
                ++steps;
                if (j < 0) { status = MP_ERR_OLOP_KEY; break; }
                const double r = rc.reward;
                if (!(0.0 <= r && r <= 1.0)) { status = MP_ERR_REWARD_RANGE; break; } // olop.py:133-134
                const int child = fc + j;
                if (lane == 0) { // OLOPNode.update (olop.py:132-142)
                    OlopNode c = N[child];
                    if (rc.flags & done_bit) c.done = 1;
                    c.cum += c.done ? 0.0 : r;
                    c.count += 1;
                    N[child] = c;
                    path[h + 1] = child;
                }
                node = child;
                __syncthreads();
            }
            if (status != MP_OK) break;
            // compute_reward_ucb (olop.py:144-163) of the path nodes, one lane each; other bound types keep mu_ucb = inf
            if (p.kl) {
                const double thr = p.thr[e];
                for (int i = 1 + lane; i <= L; i += 64) {
                    OlopNode *c = N + path[i];
                    c->mu = kl_upper_bound<false>(c->cum, c->count, thr);
                }
            }
            __syncthreads();
            // backup_to_root (olop.py:182-193), from the depth-L node up
            for (int h = L; h >= 0; --h) {
                const OlopNode nd = N[path[h]];
                double v;
                if (nd.n_children > 0) v = nd.mu + p.gamma * olop_amax(V + nd.first_child, nd.n_children, lane);
                else v = nd.mu;
                if (lane == 0) V[path[h]] = v;
                __syncthreads();
            }
        }
        // get_plan (abstract.py:143-156) with OLOPNode.selection_rule (olop.py:126-130)
        int len = 0;
        if (status == MP_OK) {
            int node = 0;
            for (;;) {
                const OlopNode nd = N[node];
                if (nd.n_children == 0) break;
                int cmax = -1;
                for (int i = lane; i < nd.n_children; i += 64) cmax = max(cmax, N[nd.first_child + i].count);
                for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
                const int j = olop_first_max(V + nd.first_child, N + nd.first_child, nd.n_children, lane, cmax);
                node = nd.first_child + j;
                if (lane == 0 && p.plans && len < p.max_plan_len) p.plans[(long)root * p.max_plan_len + len] = N[node].action;
                ++len;
            }
        }
        if (lane == 0) {
            gen.store(p.rng + (long)root * 6);
            if (p.plans)
                for (int i = len; i < p.max_plan_len; ++i) p.plans[(long)root * p.max_plan_len + i] = -1;
            if (p.plan_len) p.plan_len[root] = len;
            if (p.status) p.status[root] = status;
            if (p.env_steps) p.env_steps[root] = steps;
            if (p.root_value) p.root_value[root] = V[0];
            p.n_nodes_out[root] = n_nodes;
        }
        __syncthreads();
    }
}

// ---- OLOP on a stochastic finite MDP (mp_olop_plan_stochastic): dense [S,A,S] and sparse [S,A,B] models.
// A node is an action sequence and may be reached in many states, so the state belongs to the EPISODE: a wave-uniform value
// carried down the walk (the clone of olop.py:98), never read from a node (a node's `state` is the root's at node 0, -1 below).
//   * the clone is re-seeded per episode (state.seed(np_random.randint(2**30)), olop.py:73): numpy's SeedSequence -> PCG64
//     seeding on the 30-bit draw (seed_sequence.hpp), and the model steps draw from THAT generator, one double a step;
//   * a step is the ballot row search of brue.hip: #{j : thr_j <= k} over the model's integer thresholds ceil(cdf * 2^53),
//     64 per ballot, leaving at the first incomplete one;
//   * an expansion lists the actions of the clone's CURRENT state (the availability row, or every action): the children of a
//     node are fixed there, and a later episode that reaches the node in another state steps whichever child the bounds
//     select, listed in that state or not (the reference does, olop.py:84-88: the model has a row for every action);
//   * `done` is what the step reports -- the model's rule on the source or the next state -- and sticks to the NODE (:136-139).
// Selection, bounds, backup and get_plan are those of olop_kernel, through the same functions.
struct OlopStochArgs {
    int n_roots, A, M, L, cap, done_on_next, kl, cont, keep, grid, max_plan_len, mode, W;
    double gamma;
    const Rec *rec;          // (wave_mdp's view of a finite MDP; not read: the model is dense or sparse)
    const uint64_t *thr;     // dense [S*A][S] / sparse [S*A][B]: ceil(cdf * 2^53)
    const int32_t *nxt;      // sparse: successors [S*A][B]
    const double *R;         // reward [S*A]
    const uint8_t *term;     // terminal [S] or nullptr
    const uint8_t *avail;    // [S*A] actions the env lists, or nullptr: all
    const int32_t *root_state;
    const double *bthr;      // [M]     the bound's threshold of episode e
    const double *vinit;     // [L + 1] (1 - gamma ** (L + 1 - d)) / (1 - gamma)
    uint64_t *rng;
    OlopNode *nodes;         // [slots][cap]
    double *vu;              // [slots][cap] value_upper
    int32_t *n_nodes_out;
    int32_t *plans, *plan_len, *status;
    double *root_value;
    int64_t *env_steps;
};

__global__ __launch_bounds__(64) void olop_stoch_kernel(OlopStochArgs p)
{
    extern __shared__ int32_t path[]; // [L + 1] node ids of the episode's walk
    const int lane = threadIdx.x, A = p.A, L = p.L, W = p.W;
    const double mu0 = p.kl ? 1.0 : (double)INFINITY; // olop.py:105-108
    for (int root = blockIdx.x; root < p.n_roots; root += p.grid) {
        const long slot = p.keep ? root : (root == 0 ? p.grid : blockIdx.x);
        OlopNode *N = p.nodes + slot * p.cap;
        double *V = p.vu + slot * p.cap;
        const int s_root = p.root_state[root];
        if (lane == 0) {
            OlopNode r;
            r.cum = 0.0; r.mu = mu0; r.count = 0; r.state = s_root; r.parent = -1; r.first_child = -1;
            r.n_children = 0; r.action = -1; r.depth = 0; r.done = 0;
            N[0] = r;
            V[0] = p.vinit[0];
        }
        __syncthreads();
        Pcg64 gen;
        gen.load(p.rng + (long)root * 6);
        int n_nodes = 1, status = MP_OK;
        long steps = 0;
        for (int e = 0; e < p.M && status == MP_OK; ++e) {
            const uint32_t x = gen.below(1u << 30); // state.seed(self.np_random.randint(2**30)), olop.py:73
            Pcg64U eg;                              // Generator(PCG64(SeedSequence(x))) of the clone
            {
                uint64_t rec6[6];
                seed_sequence_record(&x, 1, rec6);
                eg.s_hi = Pcg64U::uni(rec6[0]); eg.s_lo = Pcg64U::uni(rec6[1]);
                eg.inc_hi = Pcg64U::uni(rec6[2]); eg.inc_lo = Pcg64U::uni(rec6[3]);
                eg.has_uint32 = eg.uinteger = 0;
            }
            int node = 0, s = s_root;               // the clone's state: the episode's, not the node's
            if (lane == 0) path[0] = 0;
            for (int h = 0; h < L; ++h) {
                const OlopNode nd = N[node];
                int fc = nd.first_child, k = nd.n_children, j, act;
                if (k == 0) {
                    // OLOPNode.expand (olop.py:165-180): the actions listed in the clone's current state, in listing order
                    const uint8_t *row = p.avail ? p.avail + (long)s * A : nullptr;
                    int rank0 = -1, pos0 = 0;
                    fc = n_nodes;
                    for (int a0 = 0; a0 < A; a0 += 64) {
                        const int a = a0 + lane;
                        const bool av = a < A && (!row || row[a] != 0);
                        const unsigned long long bal = olop_ballot(av);
                        const int pos = pos0 + __popcll(bal & ((1ull << lane) - 1ull));
                        if (av) {
                            OlopNode c;
                            c.cum = 0.0; c.mu = mu0; c.count = 0; c.state = -1; c.parent = node; c.first_child = -1;
                            c.n_children = 0; c.action = a; c.depth = nd.depth + 1; c.done = 0;
                            N[fc + pos] = c;
                            V[fc + pos] = p.vinit[nd.depth + 1];
                        }
                        if (p.cont >= a0 && p.cont < a0 + 64 && ((bal >> (p.cont - a0)) & 1ull))
                            rank0 = pos0 + __popcll(bal & ((1ull << (p.cont - a0)) - 1ull));
                        pos0 += __popcll(bal);
                    }
                    k = pos0;
                    if (lane == 0) { N[node].first_child = fc; N[node].n_children = k; }
                    n_nodes += k;
                    __syncthreads();
                    if (p.cont < 0) { // np_random.choice(list(children))
                        j = (int)gen.below((uint32_t)k);
                        act = N[fc + j].action;
                    } else { // action 0 (in the env's numbering): KeyError when it is not a child
                        j = rank0;
                        act = p.cont;
                    }
                } else {
                    j = olop_first_max(V + fc, N + fc, k, lane, -1);
                    act = N[fc + j].action;
                }
                // the model step (every step is taken: the reference stops neither at done nor at an unlisted action)
                const long sa = (long)s * A + act;
                const uint64_t u = eg.next64() >> 11;              // Generator.random() of the clone's generator
                const uint64_t *trow = p.thr + sa * W;
                int lo = 0;                                        // searchsorted(cdf, u, 'right') = #{j : thr_j <= u}
                for (int j0 = 0; j0 < W; j0 += 64) {
                    const int jj = j0 + lane;
                    const unsigned long long bal = olop_ballot(jj < W && trow[jj] <= u);
                    lo += __popcll(bal);
                    if (bal != ~0ull) break;
                }
                if (lo >= W) lo = W - 1;                           // (u < 1 = cdf[-1]: not reached)
                const int sn = p.mode == MP_MODE_SPARSE ? p.nxt[sa * W + lo] : lo;
                const double r = p.R[sa];
                const bool step_done = p.term ? (p.done_on_next ? p.term[sn] != 0 : p.term[s] != 0) : false;
                ++steps;
                if (j < 0) { status = MP_ERR_OLOP_KEY; break; }
                if (!(0.0 <= r && r <= 1.0)) { status = MP_ERR_REWARD_RANGE; break; } // olop.py:133-134
                const int child = fc + j;
                if (lane == 0) { // OLOPNode.update (olop.py:132-142)
                    OlopNode c = N[child];
                    if (step_done) c.done = 1;
                    c.cum += c.done ? 0.0 : r;
                    c.count += 1;
                    N[child] = c;
                    path[h + 1] = child;
                }
                node = child; s = sn;
                __syncthreads();
            }
            if (status != MP_OK) break;
            // compute_reward_ucb (olop.py:144-163) of the path nodes, one lane each; other bound types keep mu_ucb = inf
            if (p.kl) {
                const double thr = p.bthr[e];
                for (int i = 1 + lane; i <= L; i += 64) {
                    OlopNode *c = N + path[i];
                    c->mu = kl_upper_bound<false>(c->cum, c->count, thr);
                }
            }
            __syncthreads();
            // backup_to_root (olop.py:182-193), from the depth-L node up
            for (int h = L; h >= 0; --h) {
                const OlopNode nd = N[path[h]];
                double v;
                if (nd.n_children > 0) v = nd.mu + p.gamma * olop_amax(V + nd.first_child, nd.n_children, lane);
                else v = nd.mu;
                if (lane == 0) V[path[h]] = v;
                __syncthreads();
            }
        }
        // get_plan (abstract.py:143-156) with OLOPNode.selection_rule (olop.py:126-130)
        int len = 0;
        if (status == MP_OK) {
            int node = 0;
            for (;;) {
                const OlopNode nd = N[node];
                if (nd.n_children == 0) break;
                int cmax = -1;
                for (int i = lane; i < nd.n_children; i += 64) cmax = max(cmax, N[nd.first_child + i].count);
                for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
                const int j = olop_first_max(V + nd.first_child, N + nd.first_child, nd.n_children, lane, cmax);
                node = nd.first_child + j;
                if (lane == 0 && p.plans && len < p.max_plan_len) p.plans[(long)root * p.max_plan_len + len] = N[node].action;
                ++len;
            }
        }
        if (lane == 0) {
            gen.store(p.rng + (long)root * 6);
            if (p.plans)
                for (int i = len; i < p.max_plan_len; ++i) p.plans[(long)root * p.max_plan_len + i] = -1;
            if (p.plan_len) p.plan_len[root] = len;
            if (p.status) p.status[root] = status;
            if (p.env_steps) p.env_steps[root] = steps;
            if (p.root_value) p.root_value[root] = V[0];
            p.n_nodes_out[root] = n_nodes;
        }
        __syncthreads();
    }
}

// mp_selftest_olop_bound: what the device computes for the functions of kl_bound.hpp, one input per lane of 64-lane workgroups --
// the lanes of a wave run different iteration counts, as the path nodes of an episode do in olop_kernel.
__global__ __launch_bounds__(64) void olop_bound_selftest_kernel(int n, int what, const double *__restrict__ x,
                                                                 const double *__restrict__ y, const int32_t *__restrict__ count,
                                                                 double *__restrict__ out, int32_t *__restrict__ iterations,
                                                                 int32_t *__restrict__ decisions)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    if (what == 0) {
        int its, mask;
        out[i] = kl_upper_bound<true>(x[i], count[i], y[i], &its, &mask);
        iterations[i] = its;
        decisions[i] = mask;
    } else if (what == 3) { // the lower bound (MDP-GapE's mu_lcb), same outputs
        int its, mask;
        out[i] = kl_upper_bound<true, true>(x[i], count[i], y[i], &its, &mask);
        iterations[i] = its;
        decisions[i] = mask;
    } else if (what == 1) out[i] = bernoulli_kl(x[i], y[i]);
    else out[i] = log(x[i]);
}

} // namespace mp

using namespace mp;

extern "C" {

extern "C++" {
namespace {
// mp_olop_plan (each = false: `root_state` holds states of the model) and mp_olop_plan_models (each = true: it holds the GLOBAL
// states globalize_roots_arg made of the (model_index, local state) pairs; the form is each_form's)
int olop_plan_impl(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes, int32_t horizon,
                   double gamma, int32_t bound_type, int32_t continuation, const double *thresholds,
                   const double *value_upper_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len,
                   double *root_value, int64_t *env_steps, int32_t *status, int32_t mem, bool each)
{
    if (!ctx || !model || !root_state || !rng_state || !value_upper_init) return fail(MP_ERR_ARG, "mp_olop_plan: NULL argument");
    int rmem;
    MP_TRY(wave_mem("mp_olop_plan", &mem, &rmem));
    if (model->mode != MP_MODE_DETERMINISTIC)
        return fail(MP_ERR_MODE, "mp_olop_plan: model mode %d is not a deterministic table", model->mode);
    const int A = model->A;
    if (n_roots < 1 || episodes < 0 || horizon < 0 || horizon > 16384 || max_plan_len < 0)
        return fail(MP_ERR_ARG, "mp_olop_plan: bad sizes");
    if (bound_type == 1 && episodes > 0 && !thresholds) return fail(MP_ERR_ARG, "mp_olop_plan: thresholds are NULL");
    if (continuation >= A) return fail(MP_ERR_ARG, "mp_olop_plan: continuation action %d out of range", continuation);
    MP_TRY(wave_roots(ctx, "mp_olop_plan", root_state, n_roots, model->S, mem));
    const long cap = 1 + (long)episodes * horizon * A;
    if (cap > (1L << 30)) return fail(MP_ERR_ARG, "mp_olop_plan: %ld nodes per tree", cap);

    // one table: thresholds [M] then value_upper_init [L + 1] (host pointers; the values the reference's Python computes)
    std::vector<double> tab((size_t)episodes + horizon + 1);
    for (int e = 0; e < episodes; ++e) tab[e] = bound_type == 1 ? thresholds[e] : 0.0;
    for (int d = 0; d <= horizon; ++d) tab[(size_t)episodes + d] = value_upper_init[d];
    double *d_tab = nullptr;
    MP_TRY(upload_tables(ctx, 40, tab, &d_tab));

    OlopArgs a;
    a.Sb = model->Sb > 0 ? model->Sb : model->S;
    // (the global form is the launch mp_olop_plan always made: CUs * 32 wavefronts at most, path[] in LDS)
    const int cus = ctx->prop.multiProcessorCount;
    const EachForm form = each ? each_form(EACH_OLOP, a.Sb, A, horizon, n_roots, cus) : each_form_global(EACH_OLOP, horizon, n_roots, cus);
    a.n_roots = n_roots; a.A = A; a.M = episodes; a.L = horizon; a.cap = (int)cap; a.done_on_next = model->done_on_next;
    a.kl = bound_type == 1; a.cont = continuation; a.max_plan_len = max_plan_len; a.gamma = gamma;
    a.grid = form.grid; a.rec = model->rec; a.thr = d_tab; a.vinit = d_tab + episodes;
    MP_TRY(wave_tree(ctx, 5, n_roots, A, cap, 1, kOlopKeepBytes, a.grid + 1, a.grid, &a.nodes, &a.vu, &a.n_nodes_out, &a.keep));
    WaveIo io(mem, rmem, n_roots, root_state, &a.root_state, rng_state, &a.rng);
    io.add(WS_IO3, plans, &a.plans, (size_t)max_plan_len);
    io.add(WS_IO4, plan_len, &a.plan_len);
    io.add(WS_IO5, root_value, &a.root_value);
    io.add(WS_IO7, status, &a.status);
    io.add(WS_IO8, env_steps, &a.env_steps);
    MP_TRY(wave_stage(ctx, io));
    MP_TRY(wave_launch(ctx, form.lds ? olop_kernel<true> : olop_kernel<false>, a.grid, form.lds_bytes(),
                       each ? each_form_name(EACH_OLOP, form.lds, a.keep) : olop_form_name(a.keep), a));
    return wave_unstage(ctx, io);
}
} // namespace
} // extern "C++"

int mp_olop_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes, int32_t horizon,
                 double gamma, int32_t bound_type, int32_t continuation, const double *thresholds,
                 const double *value_upper_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len,
                 double *root_value, int64_t *env_steps, int32_t *status, int32_t mem)
{
    return olop_plan_impl(ctx, model, n_roots, root_state, episodes, horizon, gamma, bound_type, continuation, thresholds,
                          value_upper_init, rng_state, max_plan_len, plans, plan_len, root_value, env_steps, status, mem, false);
}

int mp_olop_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                        int32_t episodes, int32_t horizon, double gamma, int32_t bound_type, int32_t continuation,
                        const double *thresholds, const double *value_upper_init, uint64_t *rng_state, int32_t max_plan_len,
                        int32_t *plans, int32_t *plan_len, double *root_value, int64_t *env_steps, int32_t *status, int32_t mem)
{
    if (!mem_valid(mem)) return fail(MP_ERR_ARG, "mp_olop_plan_models: unknown mem flags %d", mem);
    std::vector<int32_t> tmp;
    const int32_t *global = nullptr;
    MP_TRY(globalize_roots_arg(ctx, model, n_roots, model_index, root_state, mem, tmp, &global));
    return olop_plan_impl(ctx, model, n_roots, global, episodes, horizon, gamma, bound_type, continuation, thresholds,
                          value_upper_init, rng_state, max_plan_len, plans, plan_len, root_value, env_steps, status, mem, true);
}

int mp_olop_plan_stochastic(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes,
                            int32_t horizon, double gamma, int32_t bound_type, int32_t continuation, const double *thresholds,
                            const double *value_upper_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                            int32_t *plan_len, double *root_value, int64_t *env_steps, int32_t *status, int32_t mem)
{
    const char *const who = "mp_olop_plan_stochastic";
    if (!ctx || !model || !root_state || !rng_state || !value_upper_init) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    int rmem;
    MP_TRY(wave_mem(who, &mem, &rmem));
    if (model->mode == MP_MODE_DETERMINISTIC)
        return fail(MP_ERR_MODE, "%s: a deterministic table is planned on by mp_olop_plan", who);
    MP_TRY(wave_mdp_check(who, model, false));
    const int A = model->A;
    if (n_roots < 1 || episodes < 0 || horizon < 0 || horizon > 16384 || max_plan_len < 0 || A < 1)
        return fail(MP_ERR_ARG, "%s: bad sizes", who);
    if (bound_type == 1 && episodes > 0 && !thresholds) return fail(MP_ERR_ARG, "%s: thresholds are NULL", who);
    if (continuation >= A) return fail(MP_ERR_ARG, "%s: continuation action %d out of range", who, continuation);
    MP_TRY(wave_roots(ctx, who, root_state, n_roots, model->S, mem));
    const long cap = 1 + (long)episodes * horizon * A;
    if (cap > (1L << 30)) return fail(MP_ERR_ARG, "%s: %ld nodes per tree", who, cap);
    OlopStochArgs a;
    MP_TRY(wave_mdp(ctx, who, model, &a));

    // one table: thresholds [M] then value_upper_init [L + 1] (host pointers; the values the reference's Python computes)
    std::vector<double> tab((size_t)episodes + horizon + 1);
    for (int e = 0; e < episodes; ++e) tab[e] = bound_type == 1 ? thresholds[e] : 0.0;
    for (int d = 0; d <= horizon; ++d) tab[(size_t)episodes + d] = value_upper_init[d];
    double *d_tab = nullptr;
    MP_TRY(upload_tables(ctx, 40, tab, &d_tab));

    // (the launch of mp_olop_plan: CUs * 32 wavefronts at most, path[] in LDS)
    const EachForm form = each_form_global(EACH_OLOP, horizon, n_roots, ctx->prop.multiProcessorCount);
    a.n_roots = n_roots; a.A = A; a.M = episodes; a.L = horizon; a.cap = (int)cap; a.done_on_next = model->done_on_next;
    a.kl = bound_type == 1; a.cont = continuation; a.max_plan_len = max_plan_len; a.gamma = gamma;
    a.grid = form.grid; a.term = model->term; a.avail = model->masked ? model->avail : nullptr;
    a.bthr = d_tab; a.vinit = d_tab + episodes;
    MP_TRY(wave_tree(ctx, 5, n_roots, A, cap, 1, kOlopKeepBytes, a.grid + 1, a.grid, &a.nodes, &a.vu, &a.n_nodes_out, &a.keep));
    WaveIo io(mem, rmem, n_roots, root_state, &a.root_state, rng_state, &a.rng);
    io.add(WS_IO3, plans, &a.plans, (size_t)max_plan_len);
    io.add(WS_IO4, plan_len, &a.plan_len);
    io.add(WS_IO5, root_value, &a.root_value);
    io.add(WS_IO7, status, &a.status);
    io.add(WS_IO8, env_steps, &a.env_steps);
    MP_TRY(wave_stage(ctx, io));
    MP_TRY(wave_launch(ctx, olop_stoch_kernel, a.grid, form.lds_bytes(), olop_stoch_form_name(model->mode == MP_MODE_SPARSE), a));
    return wave_unstage(ctx, io);
}

const char *mp_olop_stoch_form_names(void)
{
    static const std::string names = std::string(olop_stoch_form_name(false).s) + "\n" + olop_stoch_form_name(true).s;
    return names.c_str();
}

int mp_olop_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *action,
                        int32_t *depth, int64_t *count, double *cumulative_reward, double *mu_ucb, double *value_upper,
                        uint8_t *done, int32_t *state)
{
    int32_t slot, n;
    MP_TRY(wave_export_begin(ctx, 5, "mp_olop_tree_export", "mp_olop_plan", root, &slot, &n));
    if (n > cap) return fail(MP_ERR_ARG, "mp_olop_tree_export: capacity %d < %d nodes", cap, n);
    std::vector<OlopNode> na((size_t)n);
    std::vector<double> vu((size_t)n);
    MP_TRY(wave_pull(ctx, WS_TREE0, slot, n, sizeof(OlopNode), na.data()));
    MP_TRY(wave_pull(ctx, WS_TREE1, slot, n, sizeof(double), vu.data()));
    for (int i = 0; i < n; ++i) {
        if (parent) parent[i] = na[i].parent;
        if (action) action[i] = na[i].action;
        if (depth) depth[i] = na[i].depth;
        if (count) count[i] = na[i].count;
        if (cumulative_reward) cumulative_reward[i] = na[i].cum;
        if (mu_ucb) mu_ucb[i] = na[i].mu;
        if (value_upper) value_upper[i] = vu[i];
        if (done) done[i] = (uint8_t)na[i].done;
        if (state) state[i] = na[i].state;
    }
    if (n_nodes) *n_nodes = n;
    return MP_OK;
}

int mp_selftest_olop_bound(mp_ctx *ctx, int32_t what, int32_t n, const double *x, const double *y, const int32_t *count,
                           double *out, int32_t *iterations, int32_t *decisions)
{
    const bool traced = what == 0 || what == 3; // the two bounds: counts in, iterations and decisions out
    if (!ctx || n < 1 || what < 0 || what > 3 || !x || !out || (what != 2 && !y) || (traced && (!count || !iterations || !decisions)))
        return fail(MP_ERR_ARG, "mp_selftest_olop_bound: bad argument");
    MP_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    double *d = nullptr; // x, y, out [n] doubles, then count, iterations, decisions [n] int32
    MP_HIP(hipMalloc(&d, N * 3 * sizeof(double) + N * 3 * sizeof(int32_t)));
    int32_t *di = reinterpret_cast<int32_t *>(d + 3 * N);
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(d, x, N * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && what != 2) e = hipMemcpyAsync(d + N, y, N * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && traced) e = hipMemcpyAsync(di, count, N * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mp::olop_bound_selftest_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, n, what, d, d + N, di,
                           d + 2 * N, di + N, di + 2 * N);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + 2 * N, N * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && traced) e = hipMemcpyAsync(iterations, di + N, N * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && traced) e = hipMemcpyAsync(decisions, di + 2 * N, N * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(d);
    MP_HIP(e);
    MP_HIP(e2);
    return MP_OK;
}

} // extern "C"
