// gape_stoch.hip -- MDP-GapE with a KL confidence region over every chance node's next-state distribution
// (tree_search/mdp_gape.py:60-110, :252-313; utils.py:292-342), for max_next_states_count K in 1..32 on deterministic tables
// and on dense [S,A,S] / sparse [S,A,B] models.  gape.hip keeps the corner K = 1 on deterministic tables (mp_gape_plan).
//
// Mapping as gape.hip: ONE ROOT PER WAVEFRONT (a 64-lane workgroup), the workgroups striding over the roots.  What differs:
//   * the clone is re-seeded per episode (state.seed(np_random.randint(2**30)), :67): Generator(PCG64(SeedSequence(x))) made on
//     the device (seed_sequence.hpp), and a step of a dense / sparse model draws one double of it and finds the next state by the
//     ballot row search over ceil(cdf * 2^53), as olop_stoch_kernel.  A deterministic table reads no draw, so none is made;
//   * a decision node belongs to ONE observation: its state is the record's, and expand lists that state's actions;
//   * a chance node gets K placeholder decision children at its first get_child (:267-270), K contiguous records.  The j-th
//     state observed takes placeholder j, the lowest left (:277-285), so with m states observed the reference's dict --
//     placeholders left in number order, then the observed states by first observation -- is the records m .. K-1, 0 .. m-1:
//     lane i reads record (i + m) mod K, two contiguous runs.  The lookup of an observation is one ballot over m lanes;
//   * a chance node's backup (:288-305) is the pair of transition bounds of kl_transition.hpp, the upper solve in lanes 0..31
//     and the lower solve in lanes 32..63 of the same instructions, then p @ next by the same half-wave sums.
// Decision and chance nodes are records of ONE array (GsNode) with their two values in a second one, [cap][2], which is what
// the lanes read of a node's children.  A step makes at most K decision and |A| chance records, the root |A| more:
// cap = 1 + (episodes + 2) * horizon * K  +  (1 + (episodes + 2) * horizon) * |A|.
// The KL bounds of the path's decision nodes stay deferred to after the walk, 64 at a time; thresholds by count (both tables)
// and the initial values come from the host.
// What this file has in common with gape.hip -- the result arrays, the argument checks, the capacity refusals and the tables of the
// host side; the stopping rule and the read-out of a root on the device -- is in gape_shared.hpp, the selection among a node's
// children in gape_select.hpp.  The episode loop, the listing of an expansion and the deferred bounds included, is here.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "each_host.hpp"
#include "gape_shared.hpp"
#include "kl_bound.hpp"
#include "kl_transition.hpp"
#include "seed_sequence.hpp"
#include "wave.hpp"

namespace mp {

constexpr int kGapeStochTreeKind = 9;

struct GsNode {
    double cum, mu_ucb, mu_lcb;  // a decision node's cumulative_reward, mu_ucb, mu_lcb (olop.py:109-116, mdp_gape.py:139-143)
    int32_t count;               // visits
    int32_t key;                 // decision: the observed state, -1 - i while it is placeholder_i; chance: the action (a column)
    int32_t parent, first_child, n_children;
    int32_t depth, done, kind;   // kind 0 decision, 1 chance (a chance node has its parent's depth)
    int32_t n_assigned, pad;     // chance: the children that stand for an observed state
};
static_assert(sizeof(GsNode) == 64, "GsNode layout");

struct GapeStochArgs {
    int n_roots, A, M, H, K, cap, done_on_next, uniform, n_env, keep, grid, max_plan_len, mode, W;
    double gamma, accuracy;
    const Rec *rec;          // deterministic tables
    const uint64_t *thr;     // dense [S*A][S] / sparse [S*A][B]: ceil(cdf * 2^53)
    const int32_t *nxt;      // sparse: successors [S*A][B]
    const double *R;         // reward [S*A] (dense / sparse)
    const uint8_t *term;     // terminal [S] or nullptr (dense / sparse)
    const uint8_t *avail;    // [S*A] actions the env lists, or nullptr: all (dense / sparse)
    const int32_t *root_state;
    const double *bthr;      // [M + 2] the reward bound's threshold by count - 1
    const double *tthr;      // [M + 2] transition_threshold() by count - 1 (the kernel divides by the count, :299)
    const double *vinit;     // [H + 1] (1 - gamma ** (H - d)) / (1 - gamma)
    const double *col;       // [n_env] the column of environment action a, -1 without one
    uint64_t *rng;
    GsNode *nodes;           // [slots][cap]
    double *val;             // [slots][cap][2] value_upper, value_lower of every node
    int32_t *n_nodes_out;
    GapeResults out;
    int Sb;                  // states of one MDP of a batch model (mp_gape_plan_stochastic_models); the other entry leaves it 0
};

// EACH (mp_gape_plan_stochastic_models: a batch model of deterministic tables, one MDP per root, the roots' states GLOBAL -- nodes
// keep global states, and the availability flag and the done bits are those of the global state's records).  GS_WHOLE is the
// kernel of mp_gape_plan_stochastic; GS_EACH_GLOBAL is its table branch alone on the batch model's records (a batch model has no
// dense or sparse rows); GS_EACH_LDS copies the root's own Sb * |A| records into LDS behind path[] -- before its first episode,
// and again only when a workgroup's next root sits on another MDP -- and serves both table reads, the flags of an expansion and
// the step's record, from there: a record's `next` lies inside the root's MDP (mp_model_load_table_batch checks it), so its index
// is (state - base) * |A| + a.  Everything the each forms add sits under `if constexpr`
// (profiles/gape_stoch_each_kernel_resources.txt).
enum { GS_WHOLE = 0, GS_EACH_GLOBAL = 1, GS_EACH_LDS = 2 };

template <int EACH>
__global__ __launch_bounds__(64) void gape_stoch_kernel(GapeStochArgs p)
{
    extern __shared__ int32_t path[]; // [2 * H + 1] records of the episode's walk: decision, chance, decision, ...
    const int lane = threadIdx.x, A = p.A, H = p.H, K = p.K, W = p.W;
    constexpr bool lds_model = EACH == GS_EACH_LDS;
    const bool table = EACH != GS_WHOLE || p.mode == MP_MODE_DETERMINISTIC;
    Rec *lrec = nullptr;              // [Sb * A] GS_EACH_LDS: the root's table, 16-byte aligned behind path[]
    if constexpr (lds_model) lrec = static_cast<Rec *>(__builtin_assume_aligned(path + ((2 * H + 1 + 3) & ~3), 16));
    int base = 0, loaded = -1;        // GS_EACH_LDS: first global state of the root's MDP / index of the MDP in LDS
    // the record of (GLOBAL state, action) index `sa` = state * |A| + a
    auto rec_at = [&](long sa) -> const Rec & { return lds_model ? lrec[sa - (long)base * A] : p.rec[sa]; };
    const uint32_t done_bit = p.done_on_next ? 2u : 1u;
    for (int root = blockIdx.x; root < p.n_roots; root += p.grid) {
        const long slot = p.keep ? root : (root == 0 ? p.grid : blockIdx.x);
        GsNode *N = p.nodes + slot * p.cap;
        double *V = p.val + slot * p.cap * 2;
        // GS_EACH_LDS: the root's table into LDS (the previous root's reads ended at the barrier that closes its iteration; this
        // root's begin after the one below)
        if constexpr (lds_model) {
            const int mi = p.root_state[root] / p.Sb;
            if (mi != loaded) {
                base = mi * p.Sb;
                wave_lds_records(lrec, p.rec, base, A, p.Sb, lane);
                loaded = mi;
            }
        }
        if (lane == 0) {
            GsNode r;
            r.cum = 0.0; r.mu_ucb = 1.0; r.mu_lcb = 0.0; r.count = 0; r.key = p.root_state[root]; r.parent = -1; r.first_child = -1;
            r.n_children = 0; r.depth = 0; r.done = 0; r.kind = 0; r.n_assigned = 0; r.pad = 0;
            N[0] = r;
            V[0] = p.vinit[0]; V[1] = 0.0;
        }
        __syncthreads();
        Pcg64 gen;
        gen.load(p.rng + (long)root * 6);
        int n_nodes = 1, status = MP_OK, episodes_run = 0, best = -1, challenger = -1;
        long steps = 0;

        // DecisionNode.expand (mdp_gape.py:162-170): a chance child per action the node's state lists, in listing order; *rank =
        // the position of column `col` among them, -1 when it is not listed.  -1 when the records would not fit (not reached).
        auto expand = [&](int node, int state, int depth, int col, int *rank) {
            const int fc = n_nodes;
            *rank = -1;
            if (n_nodes + A > p.cap) return -1;
            int pos0 = 0;
            for (int a0 = 0; a0 < A; a0 += 64) {
                const int a = a0 + lane;
                bool av = false;
                if (a < A) av = table ? (rec_at((long)state * A + a).flags & 4u) != 0 : (!p.avail || p.avail[(long)state * A + a] != 0);
                const unsigned long long bal = __ballot(av);
                const int pos = pos0 + __popcll(bal & ((1ull << lane) - 1ull));
                if (av) {
                    GsNode c;
                    c.cum = 0.0; c.mu_ucb = 0.0; c.mu_lcb = 0.0; c.count = 0; c.key = a; c.parent = node; c.first_child = -1;
                    c.n_children = 0; c.depth = depth; c.done = 0; c.kind = 1; c.n_assigned = 0; c.pad = 0;
                    N[fc + pos] = c;
                    V[2 * (long)(fc + pos)] = p.vinit[depth]; // a chance node has its parent's depth (mdp_gape.py:256-258)
                    V[2 * (long)(fc + pos) + 1] = 0.0;
                }
                if (col >= a0 && col < a0 + 64 && ((bal >> (col - a0)) & 1ull))
                    *rank = pos0 + __popcll(bal & ((1ull << (col - a0)) - 1ull));
                pos0 += __popcll(bal);
            }
            if (lane == 0) { N[node].first_child = fc; N[node].n_children = pos0; }
            n_nodes += pos0;
            __syncthreads();
            return pos0;
        };

        for (int e = 0; e < p.M + 2 && status == MP_OK; ++e) {
            const uint32_t x = gen.below(1u << 30); // state.seed(self.np_random.randint(2**30)), mdp_gape.py:67
            Pcg64U eg;                              // Generator(PCG64(SeedSequence(x))) of the clone
            eg.s_hi = eg.s_lo = eg.inc_hi = eg.inc_lo = 0; eg.has_uint32 = eg.uinteger = 0;
            if (!table) {
                uint64_t rec6[6];
                seed_sequence_record(&x, 1, rec6);
                eg.s_hi = Pcg64U::uni(rec6[0]); eg.s_lo = Pcg64U::uni(rec6[1]);
                eg.inc_hi = Pcg64U::uni(rec6[2]); eg.inc_lo = Pcg64U::uni(rec6[3]);
            }
            if (N[0].n_children == 0) {
                int unused;
                if (expand(0, N[0].key, 0, -1, &unused) < 0) { status = MP_ERR_ARG; break; }
            }
            int node = 0;
            if (lane == 0) path[0] = 0;
            for (int h = 0; h < H; ++h) {
                const GsNode nd = N[node];
                const int s = nd.key;
                int fc = nd.first_child, k = nd.n_children, j;
                if (node == 0) { // sampling_rule at the root: the arm best-arm identification selects (mdp_gape.py:185-187)
                    if (k < 2) { status = MP_ERR_GAPE_NO_CHALLENGER; break; } // max() of an empty list (:247)
                    gape_bai(V + 2 * (long)fc, k, lane, &j, &best, &challenger);
                } else if (k > 0) {
                    j = gape_random_argmax(V + 2 * (long)fc, k, lane, gen);
                    if (j < 0) { status = MP_ERR_ARG; break; } // a NaN bound below the root: np_random.choice([]) raises
                } else {
                    // a childless node: randint(action_space.n) over ALL actions or action 0 (:194-196), then get_child expands
                    // and gives an unlisted action up for the first listed one (:155-160)
                    const int a_env = p.uniform ? (int)gen.below((uint32_t)p.n_env) : 0;
                    const int col = a_env < p.n_env ? (int)p.col[a_env] : -1;
                    int rank;
                    fc = n_nodes;
                    k = expand(node, s, nd.depth, col, &rank);
                    if (k < 0) { status = MP_ERR_ARG; break; }
                    j = rank >= 0 ? rank : 0;
                }
                const int ch = fc + j;
                const GsNode c0 = N[ch];
                // the model step
                const long sa = (long)s * A + c0.key;
                int sn;
                double r;
                bool step_done;
                if (table) {
                    const Rec rc = rec_at(sa);
                    sn = rc.next; r = rc.reward; step_done = (rc.flags & done_bit) != 0;
                } else {
                    const uint64_t u = eg.next64() >> 11;          // Generator.random() of the clone's generator
                    const uint64_t *trow = p.thr + sa * W;
                    int lo = 0;                                    // searchsorted(cdf, u, 'right') = #{j : thr_j <= u}
                    for (int j0 = 0; j0 < W; j0 += 64) {
                        const int jj = j0 + lane;
                        const unsigned long long bal = __ballot(jj < W && trow[jj] <= u);
                        lo += __popcll(bal);
                        if (bal != ~0ull) break;
                    }
                    if (lo >= W) lo = W - 1;                       // (u < 1 = cdf[-1]: not reached)
                    sn = p.mode == MP_MODE_SPARSE ? p.nxt[sa * W + lo] : lo;
                    r = p.R[sa];
                    step_done = p.term ? (p.done_on_next ? p.term[sn] != 0 : p.term[s] != 0) : false;
                }
                ++steps;
                // ChanceNode.get_child (:272-286): the placeholders at the first call, then the observation among the assigned
                // children or the lowest placeholder left
                int dfc = c0.first_child, m = c0.n_assigned;
                if (c0.n_children == 0) {
                    if (n_nodes + K > p.cap) { status = MP_ERR_ARG; break; } // (not reached: the bound of mp_gape_plan_stochastic)
                    dfc = n_nodes;
                    if (lane < K) {
                        GsNode d;
                        d.cum = 0.0; d.mu_ucb = 1.0; d.mu_lcb = 0.0; d.count = 0; d.key = -1 - lane; d.parent = ch; d.first_child = -1;
                        d.n_children = 0; d.depth = nd.depth + 1; d.done = 0; d.kind = 0; d.n_assigned = 0; d.pad = 0;
                        N[dfc + lane] = d;
                        V[2 * (long)(dfc + lane)] = p.vinit[nd.depth + 1];
                        V[2 * (long)(dfc + lane) + 1] = 0.0;
                    }
                    n_nodes += K;
                    __syncthreads();
                }
                const unsigned long long hit = __ballot(lane < m && N[dfc + lane].key == sn);
                int dec;
                bool assigned = false;
                if (hit) dec = dfc + __ffsll((long long)hit) - 1;
                else if (m < K) { dec = dfc + m; assigned = true; }
                else { status = MP_ERR_GAPE_PLACEHOLDERS; break; } // :284-285, after the step was counted
                if (lane == 0) { // ChanceNode.update (:264-265) and what get_child did
                    GsNode c = c0;
                    c.count += 1; c.first_child = dfc; c.n_children = K; c.n_assigned = m + (assigned ? 1 : 0);
                    N[ch] = c;
                    if (assigned) N[dec].key = sn;
                    path[2 * h + 1] = ch; path[2 * h + 2] = dec;
                }
                if (!(0.0 <= r && r <= 1.0)) { status = MP_ERR_REWARD_RANGE; break; } // olop.py:133-134
                if (lane == 0) { // OLOPNode.update (olop.py:132-142)
                    GsNode d = N[dec];
                    if (step_done) d.done = 1;
                    d.cum += d.done ? 0.0 : r;
                    d.count += 1;
                    N[dec] = d;
                }
                node = dec;
                __syncthreads();
            }
            if (status != MP_OK) break;
            // compute_reward_ucb (mdp_gape.py:200-210) of the path's decision nodes: H upper bounds, then H lower bounds
            for (int t0 = 0; t0 < 2 * H; t0 += 64) {
                const int t = t0 + lane;
                if (t < 2 * H) {
                    const bool lower = t >= H;
                    GsNode *c = N + path[2 * (lower ? t - H : t) + 2];
                    const double thr = p.bthr[c->count - 1];
                    if (lower) c->mu_lcb = kl_upper_bound<false, true>(c->cum, c->count, thr);
                    else c->mu_ucb = kl_upper_bound<false, false>(c->cum, c->count, thr);
                }
            }
            __syncthreads();
            // backup_to_root (:214-226, :288-305), from the depth-H decision node up: decision, chance, decision, ...
            for (int h = H; h >= 0; --h) {
                const int id = path[2 * h];
                const GsNode nd = N[id];
                double vu = 0.0, vl = 0.0; // the depth-H node has no children
                if (nd.n_children > 0) {
                    vu = gape_amax(V + 2 * (long)nd.first_child, nd.n_children, 0, lane);
                    vl = gape_amax(V + 2 * (long)nd.first_child, nd.n_children, 1, lane);
                }
                if (lane == 0) { V[2 * (long)id] = vu; V[2 * (long)id + 1] = vl; }
                __syncthreads();
                if (h == 0) break;
                // the chance node above: lanes 0..31 solve for value_upper (f = u_next), lanes 32..63 for value_lower (f = -l_next)
                const int ch = path[2 * h - 1];
                const GsNode cn = N[ch];
                const int li = lane & 31;
                const double c = p.tthr[cn.count - 1] / (double)cn.count;
                const bool lower = lane >= 32;
                double f = 0.0, q = 0.0, next = 0.0;
                if (li < K) {
                    const long i = cn.first_child + (li + cn.n_assigned) % K; // the reference's dict order
                    const GsNode d = N[i];
                    next = lower ? d.mu_lcb + p.gamma * V[2 * i + 1] : d.mu_ucb + p.gamma * V[2 * i];
                    f = lower ? -next : next;
                    q = (double)d.count / (double)cn.count;
                }
                const double ps = kl_transition_p<false>(f, q, c, K, lane);
                const double v = kt_half_sum(li < K ? ps * next : 0.0);
                if (li == 0) V[2 * (long)ch + (lower ? 1 : 0)] = v;
                __syncthreads();
            }
            episodes_run = e + 1;
            if (gape_stop(V, N[0].first_child, N[0].n_children, lane, p.accuracy, &best, &challenger)) break;
        }
        __syncthreads();
        const int fc0 = N[0].first_child;
        gape_read_out(p.out, p.rng, root, A, p.max_plan_len, lane, V, fc0, N[0].n_children, gen, status, best, challenger, episodes_run,
                      steps, [&](int i) { return N[fc0 + i].key; }, [&](int i) { return N[fc0 + i].count; });
        if (lane == 0) p.n_nodes_out[root] = n_nodes;
        __syncthreads();
    }
}

// mp_selftest_gape_transition: problem i in half (i & 1) of workgroup i / 2
__global__ __launch_bounds__(64) void gape_transition_selftest_kernel(int n, int K, const double *__restrict__ f,
                                                                      const double *__restrict__ q, const double *__restrict__ c,
                                                                      double *__restrict__ p_star, int32_t *__restrict__ iterations,
                                                                      int32_t *__restrict__ decisions)
{
    const int lane = threadIdx.x, li = lane & 31;
    const long i = (long)blockIdx.x * 2 + (lane >> 5);
    const bool live = i < n && li < K;
    const double fv = live ? f[i * K + li] : 0.0, qv = live ? q[i * K + li] : 0.0, cv = i < n ? c[i] : 0.0;
    int its, mask;
    const double ps = kl_transition_p<true>(fv, qv, cv, K, lane, &its, &mask);
    if (live) p_star[i * K + li] = ps;
    if (i < n && li == 0) { iterations[i] = its; decisions[i] = mask; }
}

inline FormName gape_stoch_form_name(int mode, bool keep)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "gape_stoch_%s%s", mode == MP_MODE_DETERMINISTIC ? "table" : mode == MP_MODE_SPARSE ? "sparse" : "dense",
             keep ? "" : "_slots");
    return n;
}
// mp_gape_plan_stochastic_models: the root's table in LDS or read from global memory, with the `_slots` suffix.  Listed by
// mp_gape_stoch_each_form_names, part of no other list of names.
inline FormName gape_stoch_each_form_name(bool lds, bool keep)
{
    FormName n;
    snprintf(n.s, sizeof(n.s), "gape_stoch_each_%s%s", lds ? "lds" : "global", keep ? "" : "_slots");
    return n;
}

} // namespace mp

using namespace mp;

extern "C" {

extern "C++" {
namespace {
// mp_gape_plan_stochastic (model_index NULL: `root_state` holds states of the one model) and mp_gape_plan_stochastic_models (a
// batch model of deterministic tables, `root_state` LOCAL to the MDP model_index names: globalize_roots_arg makes the GLOBAL
// states the kernel plans from, and the form is each_form's)
int gape_stoch_plan_impl(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                         int32_t episodes, int32_t horizon, int32_t max_next_states, double gamma, double accuracy,
                         int32_t continuation, int32_t n_actions_env, const int32_t *action_column, const double *thr_by_count,
                         const double *transition_thr_by_count, const double *value_init, uint64_t *rng_state,
                         int32_t max_plan_len, int32_t *plans, int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps,
                         int32_t *status, double *child_lower, double *child_upper, int64_t *child_count,
                         int32_t *best_challenger, int32_t mem, bool each)
{
    const char *const who = each ? "mp_gape_plan_stochastic_models" : "mp_gape_plan_stochastic";
    if (!ctx || !model || !root_state || !rng_state || !thr_by_count || !transition_thr_by_count || !value_init ||
        (each && !model_index))
        return fail(MP_ERR_ARG, "%s: NULL argument", who);
    const int32_t mem_flags = mem;
    int rmem;
    MP_TRY(wave_mem(who, &mem, &rmem));
    if (each && model->mode != MP_MODE_DETERMINISTIC)
        return fail(MP_ERR_MODE, "%s: model mode %d is not a deterministic table (a batch model has no dense or sparse rows)", who,
                    model->mode);
    MP_TRY(wave_mdp_check(who, model, each)); // (a CartPole model is no finite MDP: MP_ERR_MODE)
    if (each && !model->table_batch)
        return fail(MP_ERR_MODE, "%s: a batch model of deterministic tables (mp_model_load_table_batch) expected", who);
    const int A = model->A, K = max_next_states;
    if (K < 1 || K > 32) return fail(MP_ERR_ARG, "%s: max_next_states_count %d is not in 1..32 (a chance node's children fill half a wavefront)", who, K);
    const GapeTables host_tab{thr_by_count, transition_thr_by_count, value_init, nullptr};
    MP_TRY(gape_check_args(who, n_roots, episodes, horizon, 8192, max_plan_len, A, n_actions_env, gamma, accuracy, host_tab,
                           continuation, action_column));
    std::vector<int32_t> global_tmp;
    if (each) MP_TRY(globalize_roots_arg(ctx, model, n_roots, model_index, root_state, mem_flags, global_tmp, &root_state));
    MP_TRY(wave_roots(ctx, who, root_state, n_roots, model->S, mem));
    // every step of every episode may give a chance node its K placeholders and expand one decision node; the root expands once
    const long long per = ((long long)episodes + 2) * horizon;
    const long long cap = 1 + per * K + (1 + per) * A;
    MP_TRY(gape_check_capacity(who, cap, sizeof(GsNode)));
    GapeStochArgs a;
    MP_TRY(wave_mdp(ctx, who, model, &a));
    GapeTables tab;
    MP_TRY(gape_upload_tables(ctx, 43, episodes, horizon, n_actions_env, action_column, host_tab, &tab));

    // the launch of mp_gape_plan with a path of 2 * horizon + 1 records in LDS
    a.Sb = each ? (model->Sb > 0 ? model->Sb : model->S) : 0;
    const int cus = ctx->prop.multiProcessorCount;
    const EachForm form = each ? each_form(EACH_GAPE_STOCH, a.Sb, A, horizon, n_roots, cus)
                               : each_form_global(EACH_GAPE_STOCH, horizon, n_roots, cus);
    a.n_roots = n_roots; a.A = A; a.M = episodes; a.H = horizon; a.K = K; a.cap = (int)cap; a.done_on_next = model->done_on_next;
    a.uniform = continuation; a.n_env = n_actions_env; a.max_plan_len = max_plan_len; a.gamma = gamma; a.accuracy = accuracy;
    a.grid = form.grid; a.term = model->term; a.avail = model->masked ? model->avail : nullptr;
    a.bthr = tab.thr; a.tthr = tab.tthr; a.vinit = tab.vinit; a.col = tab.col;
    MP_TRY(wave_tree(ctx, kGapeStochTreeKind, n_roots, A, (long)cap, 2, kGapeKeepBytes, a.grid + 1, a.grid, &a.nodes, &a.val,
                     &a.n_nodes_out, &a.keep));
    WaveIo io(mem, rmem, n_roots, root_state, &a.root_state, rng_state, &a.rng);
    gape_results_io(io, {plans, plan_len, episodes_run, status, best_challenger, env_steps, child_count, child_lower, child_upper},
                    &a.out, max_plan_len, A);
    MP_TRY(wave_stage(ctx, io));
    if (each)
        MP_TRY(wave_launch(ctx, form.lds ? gape_stoch_kernel<GS_EACH_LDS> : gape_stoch_kernel<GS_EACH_GLOBAL>, a.grid,
                           form.lds_bytes(), gape_stoch_each_form_name(form.lds, a.keep), a));
    else
        MP_TRY(wave_launch(ctx, gape_stoch_kernel<GS_WHOLE>, a.grid, form.lds_bytes(), gape_stoch_form_name(model->mode, a.keep), a));
    return wave_unstage(ctx, io);
}
} // namespace
} // extern "C++"

int mp_gape_plan_stochastic(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes,
                            int32_t horizon, int32_t max_next_states, double gamma, double accuracy, int32_t continuation,
                            int32_t n_actions_env, const int32_t *action_column, const double *thr_by_count,
                            const double *transition_thr_by_count, const double *value_init, uint64_t *rng_state,
                            int32_t max_plan_len, int32_t *plans, int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps,
                            int32_t *status, double *child_lower, double *child_upper, int64_t *child_count,
                            int32_t *best_challenger, int32_t mem)
{
    return gape_stoch_plan_impl(ctx, model, n_roots, nullptr, root_state, episodes, horizon, max_next_states, gamma, accuracy,
                                continuation, n_actions_env, action_column, thr_by_count, transition_thr_by_count, value_init,
                                rng_state, max_plan_len, plans, plan_len, episodes_run, env_steps, status, child_lower, child_upper,
                                child_count, best_challenger, mem, false);
}

int mp_gape_plan_stochastic_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index,
                                   const int32_t *root_state, int32_t episodes, int32_t horizon, int32_t max_next_states,
                                   double gamma, double accuracy, int32_t continuation, int32_t n_actions_env,
                                   const int32_t *action_column, const double *thr_by_count, const double *transition_thr_by_count,
                                   const double *value_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                                   int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps, int32_t *status,
                                   double *child_lower, double *child_upper, int64_t *child_count, int32_t *best_challenger,
                                   int32_t mem)
{
    return gape_stoch_plan_impl(ctx, model, n_roots, model_index, root_state, episodes, horizon, max_next_states, gamma, accuracy,
                                continuation, n_actions_env, action_column, thr_by_count, transition_thr_by_count, value_init,
                                rng_state, max_plan_len, plans, plan_len, episodes_run, env_steps, status, child_lower, child_upper,
                                child_count, best_challenger, mem, true);
}

const char *mp_gape_stoch_each_form_names(void)
{
    static const std::string names = [] {
        std::string out;
        for (int lds = 1; lds >= 0; --lds)
            for (int keep = 1; keep >= 0; --keep) { out += gape_stoch_each_form_name(lds != 0, keep != 0).s; out += '\n'; }
        return out;
    }();
    return names.c_str();
}

int mp_gape_stoch_each_form_info(int32_t S_each, int32_t A, int32_t horizon, int32_t n_roots, int32_t cus, int64_t *out)
{
    if (!out) return fail(MP_ERR_ARG, "mp_gape_stoch_each_form_info: NULL output");
    if (S_each < 1 || A < 1 || horizon < 1 || n_roots < 1 || cus < 1)
        return fail(MP_ERR_ARG, "mp_gape_stoch_each_form_info: bad arguments");
    const EachForm f = each_form(EACH_GAPE_STOCH, S_each, A, horizon, n_roots, cus);
    out[0] = (int64_t)f.lds_need; out[1] = f.lds ? 1 : 0; out[2] = f.grid; out[3] = (int64_t)f.lds_bytes();
    out[4] = (int64_t)kEachLdsDefaultBytes; out[5] = (int64_t)kLdsBytes;
    return MP_OK;
}

const char *mp_gape_stoch_form_names(void)
{
    static const std::string names = [] {
        std::string out;
        for (int mode : {MP_MODE_DETERMINISTIC, MP_MODE_STOCHASTIC, MP_MODE_SPARSE})
            for (int keep = 1; keep >= 0; --keep) { out += gape_stoch_form_name(mode, keep != 0).s; out += '\n'; }
        out.pop_back();
        return out;
    }();
    return names.c_str();
}

int mp_gape_stoch_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, uint8_t *kind, int32_t *parent,
                              int32_t *action, int32_t *depth, int64_t *count, double *cumulative_reward, double *mu_ucb,
                              double *mu_lcb, double *value_upper, double *value_lower, uint8_t *done, int32_t *state)
{
    const char *const who = "mp_gape_stoch_tree_export";
    int32_t slot, n;
    MP_TRY(wave_export_begin(ctx, kGapeStochTreeKind, who, "mp_gape_plan_stochastic", root, &slot, &n));
    if (n_nodes) *n_nodes = n;
    if (n > cap) return fail(MP_ERR_ARG, "%s: capacity %d < %d nodes", who, cap, n);
    std::vector<GsNode> na((size_t)n);
    std::vector<double> val((size_t)n * 2);
    MP_TRY(wave_pull(ctx, WS_TREE0, slot, n, sizeof(GsNode), na.data()));
    MP_TRY(wave_pull(ctx, WS_TREE1, slot, n, 2 * sizeof(double), val.data()));
    // breadth first, a chance node's children in the reference's dict order: the placeholders left, then the observed states
    std::vector<int32_t> order(1, 0), par(1, -1);
    order.reserve((size_t)n); par.reserve((size_t)n);
    for (size_t q = 0; q < order.size(); ++q) {
        const GsNode &r = na[order[q]];
        if (r.n_children <= 0) continue;
        if (r.first_child < 1 || (long long)r.first_child + r.n_children > n || r.n_assigned < 0 || r.n_assigned > r.n_children ||
            order.size() + (size_t)r.n_children > (size_t)n)
            return fail(MP_ERR_ARG, "%s: bad record %d", who, order[q]);
        const int rot = r.kind ? r.n_assigned : 0;
        for (int i = 0; i < r.n_children; ++i) {
            order.push_back(r.first_child + (i + rot) % r.n_children);
            par.push_back((int32_t)q);
        }
    }
    if ((int)order.size() != n) return fail(MP_ERR_ARG, "%s: %d of %d records are reachable", who, (int)order.size(), n);
    for (int q = 0; q < n; ++q) {
        const int i = order[q];
        const GsNode &r = na[i];
        const bool chance = r.kind != 0;
        if (kind) kind[q] = chance ? 1 : 0;
        if (parent) parent[q] = par[q];
        if (action) action[q] = i == 0 ? -1 : r.key;
        if (depth) depth[q] = r.depth;
        if (count) count[q] = r.count;
        if (cumulative_reward) cumulative_reward[q] = chance ? 0.0 : r.cum;
        if (mu_ucb) mu_ucb[q] = chance ? 0.0 : r.mu_ucb;
        if (mu_lcb) mu_lcb[q] = chance ? 0.0 : r.mu_lcb;
        if (value_upper) value_upper[q] = val[2 * (size_t)i];
        if (value_lower) value_lower[q] = val[2 * (size_t)i + 1];
        if (done) done[q] = chance ? 0 : (uint8_t)r.done;
        if (state) state[q] = chance ? na[r.parent].key : (r.key >= 0 ? r.key : -1);
    }
    return MP_OK;
}

int mp_selftest_gape_transition(mp_ctx *ctx, int32_t n, int32_t K, const double *f, const double *q, const double *c,
                                double *p_star, int32_t *iterations, int32_t *decisions)
{
    const char *const who = "mp_selftest_gape_transition";
    if (!ctx || !f || !q || !c || !p_star || !iterations || !decisions) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    if (n < 1 || K < 1 || K > 32) return fail(MP_ERR_ARG, "%s: n >= 1 problems of width 1..32 expected", who);
    MP_HIP(hipSetDevice(ctx->device));
    const size_t nk = (size_t)n * K, N = (size_t)n;
    double *d = nullptr; // f, q, p_star [n][K] doubles, c [n], then iterations, decisions [n] int32
    MP_HIP(hipMalloc(&d, (3 * nk + N) * sizeof(double) + 2 * N * sizeof(int32_t)));
    int32_t *di = reinterpret_cast<int32_t *>(d + 3 * nk + N);
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(d, f, nk * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + nk, q, nk * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + 3 * nk, c, N * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(gape_transition_selftest_kernel, dim3((unsigned)((N + 1) / 2)), dim3(64), 0, st, n, K, d, d + nk,
                           d + 3 * nk, d + 2 * nk, di, di + N);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(p_star, d + 2 * nk, nk * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(iterations, di, N * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(decisions, di + N, N * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(d);
    MP_HIP(e);
    MP_HIP(e2);
    return MP_OK;
}

} // extern "C"
