// brue.hip -- Best Recommendation with Uniform Exploration, BRUE (tree_search/brue.py:11-116).
//
// Mapping: ONE ROOT PER WAVEFRONT (one 64-lane workgroup), the workgroups striding over the roots, as olop.hip.  A BRUE plan
// is a sequence of rollouts of at most H uniformly random model steps from the root (brue.py:24-33), each followed by the
// reverse pass of `update` (:47-50) with one nested `estimate` descent (:52-64) per step of the rollout:
//   * rollout and descents are the serial chain; every lane holds the same (wave-uniform) state, node and generators;
//   * the lanes cover a decision node's chance children -- a row of |A| node ids per node, so get_child(action) is one load
//     and the first maximum of `value` in creation order (Python max, :58) is a lane reduction whose ties go to the smaller
//     node id (nodes are stored in creation order: the smaller id was created first);
//   * the lanes cover a chance node's outcome children: the list is walked once (key match at creation, counts for the
//     weights), child j's count lands in lane j, the divisions counts / counts.sum() and cdf / cdf[-1] run on all lanes and
//     the cumsum between them stays a sequential chain of additions in creation order -- numpy's order (:61-62);
//   * the lanes cover the row search of a sampled step: #{j : thr_j <= k} over the model's integer thresholds
//     ceil(cdf * 2^53) (uct_stoch.hip builds them per model), 64 per ballot.
// A stochastic model's clone is re-seeded per rollout (state.seed(np_random.randint(2**30)), :25): the kernel runs numpy's
// SeedSequence -> PCG64 seeding (seed_sequence.hpp) on the 30-bit draw and steps THAT generator, one double per model step.
// Nodes live in a global workspace in creation order (the reference's order of dict insertion): at most 1 + 2 * (budget + H)
// per tree, a tree per root or per workgroup (wave_host.hpp: wave_tree).  gamma ** d comes from a host table of Python `**`;
// everything else is + - * / on f64 and integer counts, in the reference's order: results are bit-exact.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "each_host.hpp"
#include "pcg64.hpp"
#include "seed_sequence.hpp"
#include "wave.hpp"
#include "wave_host.hpp"

namespace mp {

constexpr size_t kBrueKeepBytes = (size_t)1 << 30; // trees of every root kept while they fit
constexpr int kBrueMaxHorizon = 4096;              // the rollout's path sits in LDS: 16 B a step

struct BrueNode {
    double stat;      // DecisionNode.reward (brue.py:82-86) / ChanceNode.value (:104-108): running means
    int32_t count;
    int32_t key;      // chance node: the action; decision node: the observed state (-1 at the root)
    int32_t parent;
    int32_t link;     // chance node: its first outcome child (-1: none); decision node: how many chance children it has
    int32_t next;     // decision node: the next outcome child of its parent, in creation order (-1: last)
    int32_t depthc;   // depth | is_chance << 31
};
static_assert(sizeof(BrueNode) == 32, "BrueNode layout");

struct BrueArgs {
    int n_roots, A, H, budget, cap, done_on_next, mode, W, keep, grid;
    double gamma;
    const Rec *rec;          // deterministic tables
    const uint64_t *thr;     // dense [S*A][S] / sparse [S*A][B]: ceil(cdf * 2^53)
    const int32_t *nxt;      // sparse: successors [S*A][B]
    const double *R;         // dense / sparse: reward [S*A]
    const uint8_t *term;     // dense / sparse: terminal [S] or nullptr
    const int32_t *root_state;
    const double *gpow;      // [H + 1] gamma ** d
    uint64_t *rng;
    BrueNode *nodes;         // [slots][cap]
    int32_t *ctab;           // [slots][cap][A] chance child of (decision node, action), -1 = none
    int32_t *n_nodes_out;
    int32_t *plans, *status;
    double *root_value;
    int64_t *env_steps;
    int Sb;                  // LDS_MODEL: states per MDP of the batch model (a root's MDP starts at global state (s / Sb) * Sb)
};

// First maximum of `stat` over the chance children of decision node `node` in creation order (Python max, brue.py:58; also the
// np.amax of the root's selection, abstract.py:301): value and node id, wave-uniform.  Ties go to the smaller id; only ids
// above `above` take part (the root's tie-break walks its ties in creation order with it).  Returns -1 when there is none.
__device__ __forceinline__ int brue_best_child(const BrueNode *N, const int32_t *row, int A, int lane, int above, double *value)
{
    double bv = 0.0;
    int bi = -1;
    for (int a = lane; a < A; a += 64) {
        const int c = row[a];
        if (c > above) {
            const double v = N[c].stat;
            if (bi < 0 || v > bv || (v == bv && c < bi)) { bv = v; bi = c; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    *value = bv;
    return bi;
}

// m nodes of an outcome list from node `o` on: child j's id and count into lane j; `o` moves past them
__device__ __forceinline__ void brue_capture(const BrueNode *N, int &o, int m, int lane, int &id, int &cnt)
{
    for (int j = 0; j < m; ++j) {
        const BrueNode nd = N[o];
        if (lane == j) { id = o; cnt = nd.count; }
        o = nd.next;
    }
}

// LDS_MODEL (mp_brue_plan_models, one MDP per root, deterministic tables): the root's own Sb * |A| records sit in LDS behind
// rew[] and po[] (16 bytes a step: the records stay 16-byte aligned), copied before its first rollout, and the rollout's step --
// the only model read of a plan: `estimate` walks the tree -- is served from there.
template <bool LDS_MODEL>
__global__ __launch_bounds__(64) void brue_kernel(BrueArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char brue_smem[];
    double *rew = reinterpret_cast<double *>(brue_smem);           // [H] reward of the rollout's step
    int2 *po = reinterpret_cast<int2 *>(rew + p.H);                // [H] {chance node, decision node it led to}
    Rec *lrec = reinterpret_cast<Rec *>(po + p.H);                 // [Sb * A] LDS_MODEL: the root's table
    const int lane = threadIdx.x, A = p.A, H = p.H;
    for (int root = blockIdx.x; root < p.n_roots; root += p.grid) {
        const long slot = p.keep ? root : (root == 0 ? p.grid : blockIdx.x);
        BrueNode *N = p.nodes + slot * p.cap;
        int32_t *C = p.ctab + slot * p.cap * A;
        const int s_root = p.root_state[root];
        int base = 0;
        if constexpr (LDS_MODEL) {                                 // (the previous root's reads ended at the barrier closing its iteration)
            base = s_root / p.Sb * p.Sb;
            wave_lds_records(lrec, p.rec, base, A, p.Sb, lane);
        }
        if (lane == 0) {                                           // DecisionNode(parent=None), brue.py:22
            BrueNode r;
            r.stat = 0.0; r.count = 0; r.key = -1; r.parent = -1; r.link = 0; r.next = -1; r.depthc = 0;
            N[0] = r;
        }
        for (int a = lane; a < A; a += 64) C[a] = -1;
        __syncthreads();
        Pcg64U gen;
        gen.load(p.rng + (long)root * 6);
        int n_nodes = 1, status = MP_OK, left = p.budget;
        long steps = 0;
        while (left > 0 && status == MP_OK) {                      // brue.py:68-70
            // ---- rollout (:24-33) with the walk down of update (:40-44)
            const uint32_t x = gen.below(1u << 30);                // state.seed(self.np_random.randint(2**30)), :25
            Pcg64U eg;
            eg.s_hi = eg.s_lo = eg.inc_hi = eg.inc_lo = 0; eg.has_uint32 = eg.uinteger = 0;
            if (!LDS_MODEL && p.mode != MP_MODE_DETERMINISTIC) {   // Generator(PCG64(SeedSequence(x))) of the clone
                uint64_t rec6[6];
                seed_sequence_record(&x, 1, rec6);
                eg.s_hi = Pcg64U::uni(rec6[0]); eg.s_lo = Pcg64U::uni(rec6[1]);
                eg.inc_hi = Pcg64U::uni(rec6[2]); eg.inc_lo = Pcg64U::uni(rec6[3]);
            }
            int node = 0, s = s_root, len = 0, depth = 0;
            for (int h = 0; h < H; ++h) {
                if (n_nodes + 2 > p.cap) { status = MP_ERR_ARG; break; }   // (cannot happen: cap = 1 + 2 * (budget + H))
                const int a = (int)gen.below((uint32_t)A);         // np_random.randint(action_space.n), :27
                const long sa = (long)s * A + a;
                int sn;
                double r;
                bool done;
                if (LDS_MODEL || p.mode == MP_MODE_DETERMINISTIC) {
                    const Rec rc = LDS_MODEL ? lrec[(s - base) * A + a] : p.rec[sa];
                    sn = rc.next; r = rc.reward;
                    done = (rc.flags & (p.done_on_next ? 2u : 1u)) != 0;
                } else {
                    const uint64_t k = eg.next64() >> 11;          // Generator.random() of the clone's generator
                    const uint64_t *trow = p.thr + sa * p.W;
                    int lo = 0;                                    // searchsorted(cdf, u, 'right') = #{j : thr_j <= k}
                    for (int j0 = 0; j0 < p.W; j0 += 64) {
                        const int j = j0 + lane;
                        const unsigned long long bal = __ballot(j < p.W && trow[j] <= k);
                        lo += __popcll(bal);
                        if (bal != ~0ull) break;
                    }
                    if (lo >= p.W) lo = p.W - 1;                   // (u < 1 = cdf[-1]: not reached)
                    sn = p.mode == MP_MODE_SPARSE ? p.nxt[sa * p.W + lo] : lo;
                    r = p.R[sa];
                    done = p.term ? (p.done_on_next ? p.term[sn] != 0 : p.term[s] != 0) : false;
                }
                ++steps;
                // state_node.get_child(action), :93-96
                int c = C[(long)node * A + a];
                if (c < 0) {
                    c = n_nodes++;
                    if (lane == 0) {
                        BrueNode nd;
                        nd.stat = 0.0; nd.count = 0; nd.key = a; nd.parent = node; nd.link = -1; nd.next = -1;
                        nd.depthc = depth | (int)0x80000000;
                        N[c] = nd;
                        C[(long)node * A + a] = c;
                        N[node].link += 1;
                    }
                    __syncthreads();
                }
                // chance_node.get_child(next_obs), :113-116: the outcome list in creation order
                int o = N[c].link, last = -1;
                while (o >= 0) {
                    const BrueNode nd = N[o];
                    if (nd.key == sn) break;
                    last = o;
                    o = nd.next;
                }
                if (o < 0) {
                    o = n_nodes++;
                    if (lane == 0) {
                        BrueNode nd;
                        nd.stat = 0.0; nd.count = 0; nd.key = sn; nd.parent = c; nd.link = 0; nd.next = -1; nd.depthc = depth + 1;
                        N[o] = nd;
                        if (last < 0) N[c].link = o; else N[last].next = o;
                    }
                    for (int b = lane; b < A; b += 64) C[(long)o * A + b] = -1;
                    __syncthreads();
                }
                if (lane == 0) { rew[len] = r; po[len] = make_int2(c, o); }
                ++len;
                node = o; s = sn; ++depth;
                --left;                                            // self.available_budget -= 1, :31
                if (done) break;
            }
            __syncthreads();
            // ---- update (:47-50), from the last step up
            for (int i = len - 1; i >= 0; --i) {
                const int2 pr = po[i];
                const double r = rew[i];
                const int c = pr.x, o = pr.y;
                BrueNode on = N[o];
                on.count += 1;                                     // next_state_node.update(reward), :84-86
                on.stat = (double)(on.count - 1) / (double)on.count * on.stat + r / (double)on.count;
                if (lane == 0) { N[o].count = on.count; N[o].stat = on.stat; }
                __syncthreads();
                // estimate(next_state_node), :52-64
                double ret = 0.0;
                int cur = o, nk = on.link;
                for (int d = 0; d < H - (i + 1) && nk > 0; ++d) {
                    double bv;
                    const int best = brue_best_child(N, C + (long)cur * A, A, lane, -1, &bv);   // :58
                    // np_random.choice(next_states, p=counts / counts.sum()), :60-62
                    const int first = N[best].link;
                    int n = 0, id = -1, cnt = 0, w = first;
                    long total = 0;
                    while (w >= 0) {
                        const BrueNode nd = N[w];
                        if (lane == n) { id = w; cnt = nd.count; }
                        total += nd.count;
                        ++n;
                        w = nd.next;
                    }
                    const double u = (double)(gen.next64() >> 11) * (1.0 / 9007199254740992.0);
                    const double tot = (double)total;
                    double acc = 0.0;                              // cdf = p.cumsum(): sequential, in creation order
                    w = first;
                    for (int base = 0; base < n; base += 64) {
                        const int m = n - base < 64 ? n - base : 64;
                        if (n > 64) brue_capture(N, w, m, lane, id, cnt);
                        const double pj = (double)cnt / tot;
                        for (int j = 0; j < m; ++j) acc += __shfl(pj, j);
                    }
                    const double cdf_last = acc;
                    acc = 0.0;
                    w = first;
                    int chosen = -1;                               // cdf /= cdf[-1]; searchsorted(cdf, u, 'right')
                    for (int base = 0; base < n && chosen < 0; base += 64) {
                        const int m = n - base < 64 ? n - base : 64;
                        if (n > 64) brue_capture(N, w, m, lane, id, cnt);
                        const double pj = (double)cnt / tot;
                        double mine = 0.0;
                        for (int j = 0; j < m; ++j) {
                            acc += __shfl(pj, j);
                            if (lane == j) mine = acc;
                        }
                        const int le = __popcll(__ballot(lane < m && mine / cdf_last <= u));
                        if (le < m || base + m >= n) chosen = __shfl(id, le < m ? le : m - 1);   // (u < 1 = cdf[-1])
                    }
                    if (chosen < 0) break;                         // (not reached: a chance node has an outcome child)
                    const BrueNode nx = N[chosen];
                    ret += p.gpow[d] * nx.stat;                    // return_ += gamma**d * state_node.reward, :63
                    cur = chosen; nk = nx.link;
                }
                const double er = r + p.gamma * ret;               // :49
                BrueNode cn = N[c];
                cn.count += 1;                                     // chance_node.update(estimated_return), :106-108
                cn.stat = (double)(cn.count - 1) / (double)cn.count * cn.stat + er / (double)cn.count;
                if (lane == 0) { N[c].count = cn.count; N[c].stat = cn.stat; }
                __syncthreads();
            }
        }
        // ---- get_plan (:73-75): root.selection_rule() (:88-91) = random_argmax of the children's values (abstract.py:296-311)
        int plan = -1;
        double value = 0.0;
        if (status == MP_OK && N[0].link > 0) {
            double vmax;
            int pick = brue_best_child(N, C, A, lane, -1, &vmax);  // the first of the ties in creation order
            int ties = 0;
            for (int a = lane; a < A; a += 64) {
                const int c = C[a];
                if (c >= 0 && N[c].stat == vmax) ++ties;
            }
            for (int off = 32; off > 0; off >>= 1) ties += __shfl_xor(ties, off);
            int j = (int)gen.below((uint32_t)ties);                // np_random.choice(indices): a draw for two ties or more
            while (j-- > 0) {                                      // the next tie in creation order
                int bi = -1;
                for (int a = lane; a < A; a += 64) {
                    const int c = C[a];
                    if (c > pick && N[c].stat == vmax && (bi < 0 || c < bi)) bi = c;
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const int oi = __shfl_xor(bi, off);
                    if (oi >= 0 && (bi < 0 || oi < bi)) bi = oi;
                }
                if (bi < 0) break;                                 // (not reached: `ties` children hold vmax)
                pick = bi;
            }
            plan = N[pick].key;
            value = N[pick].stat;
        }
        if (lane == 0) {
            gen.store(p.rng + (long)root * 6);
            if (p.plans) p.plans[root] = plan;
            if (p.status) p.status[root] = status;
            if (p.env_steps) p.env_steps[root] = steps;
            if (p.root_value) p.root_value[root] = value;
            p.n_nodes_out[root] = n_nodes;
        }
        __syncthreads();
    }
}

} // namespace mp

using namespace mp;

extern "C" {

extern "C++" {
namespace {
// mp_brue_plan (each = false: `root_state` holds states of the one model) and mp_brue_plan_models (each = true: a batch model
// of deterministic tables; it holds the GLOBAL states globalize_roots_arg made of the (model_index, local state) pairs and the
// form is each_form's)
int brue_plan_impl(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t budget, int32_t horizon,
                   double gamma, const double *gpow, uint64_t *rng_state, int32_t *plans, double *root_value, int64_t *env_steps,
                   int32_t *status, int32_t mem, bool each)
{
    if (!ctx || !model || !root_state || !rng_state || !gpow) return fail(MP_ERR_ARG, "mp_brue_plan: NULL argument");
    int rmem;
    MP_TRY(wave_mem("mp_brue_plan", &mem, &rmem));
    MP_TRY(wave_mdp_check("mp_brue_plan", model, each));
    const int A = model->A;
    // (a rollout of no step never spends the budget: the reference loops for ever with horizon 0)
    if (n_roots < 1 || horizon < 1 || horizon > kBrueMaxHorizon || A < 1)
        return fail(MP_ERR_ARG, "mp_brue_plan: bad sizes (1 <= horizon <= %d)", kBrueMaxHorizon);
    if (budget < 0) budget = 0;
    MP_TRY(wave_roots(ctx, "mp_brue_plan", root_state, n_roots, model->S, mem));
    const long cap = 1 + 2 * ((long)budget + horizon);
    if (cap * A > (1L << 30)) return fail(MP_ERR_ARG, "mp_brue_plan: %ld nodes of %d actions per tree", cap, A);
    BrueArgs a;
    MP_TRY(wave_mdp(ctx, "mp_brue_plan", model, &a));

    std::vector<double> tab(gpow, gpow + horizon + 1);             // gamma ** d, the host's Python `**`
    double *d_tab = nullptr;
    MP_TRY(upload_tables(ctx, 41, tab, &d_tab));

    a.Sb = model->Sb > 0 ? model->Sb : model->S;
    // (the global form is the launch mp_brue_plan always made: CUs * 32 wavefronts at most, rew[] and po[] in LDS)
    const int cus = ctx->prop.multiProcessorCount;
    const EachForm form = each ? each_form(EACH_BRUE, a.Sb, A, horizon, n_roots, cus) : each_form_global(EACH_BRUE, horizon, n_roots, cus);
    a.n_roots = n_roots; a.A = A; a.H = horizon; a.budget = budget; a.cap = (int)cap; a.done_on_next = model->done_on_next;
    a.grid = form.grid; a.gamma = gamma; a.term = model->term; a.gpow = d_tab;
    MP_TRY(wave_tree(ctx, 6, n_roots, A, cap, (size_t)A, kBrueKeepBytes, a.grid + 1, a.grid, &a.nodes, &a.ctab, &a.n_nodes_out, &a.keep));
    WaveIo io(mem, rmem, n_roots, root_state, &a.root_state, rng_state, &a.rng);
    io.add(WS_IO3, plans, &a.plans);
    io.add(WS_IO5, root_value, &a.root_value);
    io.add(WS_IO7, status, &a.status);
    io.add(WS_IO8, env_steps, &a.env_steps);
    MP_TRY(wave_stage(ctx, io));
    MP_TRY(wave_launch(ctx, form.lds ? brue_kernel<true> : brue_kernel<false>, a.grid, form.lds_bytes(),
                       each ? each_form_name(EACH_BRUE, form.lds, a.keep) : brue_form_name(a.keep), a));
    return wave_unstage(ctx, io);
}
} // namespace
} // extern "C++"

int mp_brue_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t budget, int32_t horizon,
                 double gamma, const double *gpow, uint64_t *rng_state, int32_t *plans, double *root_value, int64_t *env_steps,
                 int32_t *status, int32_t mem)
{
    return brue_plan_impl(ctx, model, n_roots, root_state, budget, horizon, gamma, gpow, rng_state, plans, root_value, env_steps,
                          status, mem, false);
}

int mp_brue_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                        int32_t budget, int32_t horizon, double gamma, const double *gpow, uint64_t *rng_state, int32_t *plans,
                        double *root_value, int64_t *env_steps, int32_t *status, int32_t mem)
{
    if (!mem_valid(mem)) return fail(MP_ERR_ARG, "mp_brue_plan_models: unknown mem flags %d", mem);
    std::vector<int32_t> tmp;
    const int32_t *global = nullptr;
    MP_TRY(globalize_roots_arg(ctx, model, n_roots, model_index, root_state, mem, tmp, &global));
    return brue_plan_impl(ctx, model, n_roots, global, budget, horizon, gamma, gpow, rng_state, plans, root_value, env_steps,
                          status, mem, true);
}

int mp_brue_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *key,
                        uint8_t *is_chance, int32_t *depth, int64_t *count, double *stat)
{
    int32_t slot, n;
    MP_TRY(wave_export_begin(ctx, 6, "mp_brue_tree_export", "mp_brue_plan", root, &slot, &n));
    if (n > cap) return fail(MP_ERR_ARG, "mp_brue_tree_export: capacity %d < %d nodes", cap, n);
    std::vector<BrueNode> na((size_t)n);
    MP_TRY(wave_pull(ctx, WS_TREE0, slot, n, sizeof(BrueNode), na.data()));
    for (int i = 0; i < n; ++i) {
        if (parent) parent[i] = na[i].parent;
        if (key) key[i] = na[i].key;
        if (is_chance) is_chance[i] = na[i].depthc < 0 ? 1 : 0;
        if (depth) depth[i] = na[i].depthc & 0x7fffffff;
        if (count) count[i] = na[i].count;
        if (stat) stat[i] = na[i].stat;
    }
    if (n_nodes) *n_nodes = n;
    return MP_OK;
}

} // extern "C"
