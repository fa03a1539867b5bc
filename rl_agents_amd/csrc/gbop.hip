// gbop.hip -- GBOP, graph-based optimistic planning for stochastic MDPs (tree_search/graph_based_stochastic.py) with known
// rewards (reward threshold 0, the configs the reference ships), for many independent planners of one finite MDP: a
// deterministic table, a dense [S,A,S] or a sparse [S,A,B] model.
//
// The reference's StochasticGraphBasedPlanner keeps ONE decision node per observed state (planner.nodes, get_node,
// graph_based.py:110-116) with a lower and an upper bound of V, a count and its parents; per listed action of an expanded
// node a chance node (:133-225) with its count, its two stored bounds and max_next_states_count = K transition children:
// placeholders until a next state is observed and takes the lowest-numbered one left (:207-219).  An episode (run, :234-268)
// walks `horizon` steps by the optimistic sampling rule (:42-51: the upper backup of EVERY chance child, then random_argmax),
// records counts and rewards, and ends with a partial value iteration over the decision nodes it visited, newest first, that
// runs backwards through the graph (:89-101): a first-in-first-out list with duplicates; a popped node takes the maximum of its
// chance children's lower, then upper, backups and appends all its parents when either moved by more than `accuracy`.  A
// chance node's backup (:167-198) is max_expectation_under_constraint around the next-state frequencies (kl_transition.hpp).
// planner.nodes with every chance record outlives plan() calls and agent.reset() (:339-343 replaces `root` only): the planner
// state is a device-resident handle, as mp_gbopd is.
//
// Mapping.  One planner per WAVEFRONT (a workgroup is one wavefront; the workgroups stride over the planners).  The walk and
// the chain of pops are serial by the reference's definition, so they run as uniform code; the lanes cover
//   a chance node's children   the K <= 32 entries of one solve fill HALF a wavefront (kl_transition.hpp), so two solves run side
//                              by side: in a pop the upper and the lower backup of one chance node (independent: each reads
//                              its own bound of the graph nodes), in the sampling rule and in get_plan the same backup of two
//                              chance nodes.  A chance node never tried (count 0) returns its stored bound without a solve
//   a node's actions           the listing (ballot), both maxima of a pop, the tie draw of random_argmax
//   a node's parents           the membership scan of parents.add and the append of a popped node's parents to the queue
//   a dense / sparse row       the ballot search of the sampled next state over ceil(cdf * 2^53), as gape_stoch.hip
//
// Storage per planner, addressed by STATE and by (state, action slot): a finite MDP's graph never holds more than S decision
// nodes and S * A chance nodes, so nothing is allocated during a plan.
//   lower / upper f64 [S], index / created i32 [S], expanded u8 [S], count / visits i64 [S]   as gbopd.hip
//   par i32 [E], npar i32 [S]   parents in INSERTION order; parents[c] can only hold the states with a listed action that may
//                               lead to c: the handle counts them on the model once (in_ptr [S + 1], shared by the planners)
//   queue i32 [queue_cap], uq i32 [S]   the backup ring and the episode's update_queue
//   c_count / c_m / c_backed i32 [S*A], c_val f64 [S*A][2]   N(s,a), the children that stand for a state, that number at the
//                               last backup (`next_states`), value_upper / value_lower
//   k_state / k_count i32, k_cum / k_mu / k_lcb / pp / pm f64 [S*A][K]   child SLOT j: the state (-1 - j while placeholder_j),
//                               N(s,a,s'), the reward sum, mu_ucb, mu_lcb; p_plus / p_minus in the dict order of their backup
// With m states observed the reference's dict holds the slots m .. K-1, 0 .. m-1 (a popped placeholder is re-inserted at the
// end): entry i of a solve reads slot (i + m) mod K.  The records of a state are initialised when it is expanded.
// While 16 * S bytes fit (MP_GBOP_LDS_BYTES, default 16 KiB) both bounds of the graph nodes live in LDS for the plan, as in
// gbopd_kernel; the chance records, which a backup streams through once, stay in global memory.
#include <math.h>
#include <stdlib.h>

#include <new>
#include <string>
#include <vector>

#include "common.hpp"
#include "graph_shared.hpp"
#include "kl_transition.hpp"
#include "opd_closing.hpp"
#include "pcg64.hpp"
#include "seed_sequence.hpp"
#include "wave.hpp"

struct mp_gbop : mp::GraphHandle {
    int K = 0;
    int64_t steps_bound = 0;    // no count of any planner exceeds it: the steps of every plan call so far
    double *c_val = nullptr, *k_cum = nullptr, *k_mu = nullptr, *k_lcb = nullptr, *pp = nullptr, *pm = nullptr;
    int32_t *uq = nullptr, *c_count = nullptr, *c_m = nullptr, *c_backed = nullptr, *k_state = nullptr, *k_count = nullptr;
    int64_t *count = nullptr;
    std::vector<uint8_t> h_listed;  // [S * A] the actions a state lists (slot = listing order)
};

namespace mp {

struct GbopArgs {
    int n, S, A, K, M, H, qcap, mode, W, plan_steps, n_counts;
    long E, max_pops;
    double gamma, vmax, accuracy;
    const Rec *rec;          // deterministic tables
    const uint64_t *thr;     // dense [S*A][S] / sparse [S*A][B]: ceil(cdf * 2^53)
    const int32_t *nxt;      // sparse: successors [S*A][B]
    const double *R;         // reward [S*A] (dense / sparse)
    const uint8_t *avail;    // [S*A] actions the env lists, or nullptr: all (dense / sparse)
    const int32_t *in_ptr;
    const int32_t *root_state;
    const double *rthr, *tthr;   // [n_counts] the reward / transition threshold by count - 1
    uint64_t *rng;
    double *lower, *upper, *c_val, *k_cum, *k_mu, *k_lcb, *pp, *pm;
    int32_t *index, *npar, *created, *par, *queue, *uq, *n_created, *failed, *root_of;
    int32_t *c_count, *c_m, *c_backed, *k_state, *k_count;
    uint8_t *expanded;
    int64_t *count, *visits, *n_obs;
    int32_t *action, *key, *plan_len, *status;
    double *root_lower, *root_upper;
    int64_t *env_steps, *pops;
};

template <bool LDSV>
__global__ __launch_bounds__(64) void gbop_kernel(GbopArgs p)
{
    extern __shared__ __attribute__((aligned(16))) double lds_v[];
    const int lane = threadIdx.x, li = lane & 31;
    const bool l0 = lane == 0, hi = lane >= 32;
    const int S = p.S, A = p.A, K = p.K;
    const bool table = p.mode == MP_MODE_DETERMINISTIC;
    const double gamma = p.gamma, ninf = -INFINITY;
    const unsigned qmask = (unsigned)p.qcap - 1u;

    for (int r = blockIdx.x; r < p.n; r += gridDim.x) {
        const long sb = (long)r * S, cb = sb * A, kb = cb * K;
        const int s0 = p.root_state[r];
        int status = p.failed[r]; // failed for good in an earlier call: the code it failed with
        if (status == MP_OK && (unsigned)s0 >= (unsigned)S) status = MP_ERR_ARG;
        if (status != MP_OK) {
            if (l0) {
                if (p.action) p.action[r] = -1;
                if (p.key) p.key[r] = 0;
                graph_refuse(r, status, p.plan_len, p.status, p.root_lower, p.root_upper, p.env_steps, p.pops);
            }
            continue;
        }
        __syncthreads(); // (LDS of the previous planner of this workgroup is free)
        double *const lower = LDSV ? lds_v : p.lower + sb;
        double *const upper = LDSV ? lds_v + S : p.upper + sb;
        int32_t *const index = p.index + sb, *const npar = p.npar + sb, *const created = p.created + sb, *const uq = p.uq + sb;
        uint8_t *const expanded = p.expanded + sb;
        int64_t *const count = p.count + sb, *const visits = p.visits + sb;
        int32_t *const par = p.par + (long)r * p.E;
        int32_t *const queue = p.queue + (long)r * p.qcap;
        int32_t *const c_count = p.c_count + cb, *const c_m = p.c_m + cb, *const c_backed = p.c_backed + cb;
        double *const c_val = p.c_val + 2 * cb;
        int32_t *const k_state = p.k_state + kb, *const k_count = p.k_count + kb;
        double *const k_cum = p.k_cum + kb, *const k_mu = p.k_mu + kb, *const k_lcb = p.k_lcb + kb, *const pp = p.pp + kb,
                      *const pm = p.pm + kb;

        int n_created = p.n_created[r];
        if (LDSV) graph_stage_in(p.lower, p.upper, sb, created, n_created, lower, upper, lane); // the bounds of the nodes that exist
        // graph_based.py:110-116 (every caller of it is uniform)
        auto get_node = [&](int s) {
            if (index[s] < 0) {
                if (l0) {
                    index[s] = n_created; created[n_created] = s;
                    lower[s] = 0.0; upper[s] = p.vmax;
                }
                ++n_created;
                __syncthreads();
            }
        };
        auto listed = [&](int s, int a) {
            return table ? (p.rec[(long)s * A + a].flags & 4u) != 0 : (!p.avail || p.avail[(long)s * A + a] != 0);
        };
        // GraphChanceNode.backup (:167-198) of two (chance node, field) pairs, one per half of the wavefront; sa < 0: none.
        // Writes p_plus / p_minus, the bound and `next_states`; false when a count is past the threshold table.
        auto backup2 = [&](long sa_lo, bool up_lo, long sa_hi, bool up_hi) {
            const long sa = hi ? sa_hi : sa_lo;
            const bool up = hi ? up_hi : up_lo, live = sa >= 0;
            int cnt = 0, m = 0;
            if (live) { cnt = c_count[sa]; m = c_m[sa]; }
            const bool bad = live && cnt > p.n_counts;
            const bool solve = live && cnt > 0 && !bad;
            double f = 0.0, q = 0.0, next = 0.0, c = 0.0;
            if (solve) {
                c = p.tthr[cnt - 1] / (double)cnt; // :179
                if (li < K) {
                    const long i = sa * K + (li + m) % K; // the reference's dict order
                    const int st = k_state[i];
                    const double vn = st >= 0 ? (up ? upper[st] : lower[st]) : (up ? p.vmax : 0.0);
                    next = k_mu[i] + gamma * vn;          // mu_ucb in BOTH bounds (:186, :195)
                    f = up ? next : -next;
                    q = (double)k_count[i] / (double)cnt;
                }
            }
            const double ps = kl_transition_p<false>(f, q, c, K, lane);
            const double v = kt_half_sum(li < K ? ps * next : 0.0);
            if (live && !bad) {
                if (solve) {
                    if (li < K) (up ? pp : pm)[sa * K + li] = ps;
                    if (li == 0) c_val[2 * sa + (up ? 0 : 1)] = v;
                } else if (li < K) { // :171-174: both distributions uniform, the stored bound is returned
                    pp[sa * K + li] = 1.0 / (double)K;
                    pm[sa * K + li] = 1.0 / (double)K;
                }
                if (li == 0) c_backed[sa] = m;
            }
            return !any64(bad);
        };
        // GraphDecisionNode.backup (:86-87) over the listed actions of s.  both: upper and lower of each chance node side by
        // side; else the field `up` of two chance nodes at a time.  -1: a count past the tables, else the listed actions.
        auto backup_node = [&](int s, bool both, bool up) {
            int n_listed = 0;
            bool ok = true;
            for (int a0 = 0; a0 < A; a0 += 64) {
                const int a = a0 + lane;
                unsigned long long lm = ballot64(a < A && listed(s, a));
                n_listed += __popcll(lm);
                while (lm) {
                    const long sa1 = (long)s * A + a0 + __ffsll((long long)lm) - 1;
                    lm &= lm - 1;
                    if (both) ok = backup2(sa1, true, sa1, false) && ok;
                    else {
                        long sa2 = -1;
                        if (lm) { sa2 = (long)s * A + a0 + __ffsll((long long)lm) - 1; lm &= lm - 1; }
                        ok = backup2(sa1, up, sa2, up) && ok;
                    }
                }
            }
            __syncthreads();
            return ok ? n_listed : -1;
        };
        // np.amax of the chance children's bound `which` (0 upper, 1 lower); a NaN never wins
        auto amax_listed = [&](int s, int which) {
            double m = ninf;
            for (int a = lane; a < A; a += 64)
                if (listed(s, a)) {
                    const double v = c_val[2 * ((long)s * A + a) + which];
                    m = v > m ? v : m;
                }
            return wave_max(m);
        };

        // plan(), :333: root = get_node(observation)
        get_node(s0);
        if (l0) p.root_of[r] = s0;
        Pcg64 gen;
        gen.load(p.rng + (long)r * 6);
        long steps = 0, pops_total = 0;

        for (int e = 0; e < p.M && status == MP_OK; ++e) {
            // ---- run(), :234-268
            const uint32_t x = gen.below(1u << 30); // state.seed(self.np_random.randint(2**30)), :239
            Pcg64U eg;                              // Generator(PCG64(SeedSequence(x))) of the clone
            eg.s_hi = eg.s_lo = eg.inc_hi = eg.inc_lo = 0; eg.has_uint32 = eg.uinteger = 0;
            if (!table) {
                uint64_t rec6[6];
                seed_sequence_record(&x, 1, rec6);
                eg.s_hi = Pcg64U::uni(rec6[0]); eg.s_lo = Pcg64U::uni(rec6[1]);
                eg.inc_hi = Pcg64U::uni(rec6[2]); eg.inc_lo = Pcg64U::uni(rec6[3]);
            }
            int s = s0, nq = 0;
            for (int h = 0; h < p.H; ++h) {
                // sampling_rule (:42-51): expand (:103-105, :137-150) on the first visit
                if (!expanded[s]) {
                    for (int i = lane; i < A * K; i += 64) {
                        const long j = (long)s * A * K + i;
                        k_state[j] = -1 - i % K; k_count[j] = 0;
                        k_cum[j] = 0.0; k_mu[j] = 1.0; k_lcb[j] = 0.0; pp[j] = 0.0; pm[j] = 0.0;
                    }
                    bool any_listed = false;
                    for (int a = lane; a < A; a += 64) {
                        const long sa = (long)s * A + a;
                        c_count[sa] = 0; c_m[sa] = 0; c_backed[sa] = -1;
                        c_val[2 * sa] = p.vmax; c_val[2 * sa + 1] = 0.0; // GraphNode.__init__, graph_based.py:17-18
                        any_listed = any_listed || listed(s, a);
                    }
                    // a node no action is listed for: np.amax([]) in random_argmax raises ValueError
                    if (!any64(any_listed)) { status = MP_ERR_GBOPD_NO_ACTION; break; }
                    if (l0) expanded[s] = 1;
                    __syncthreads();
                }
                if (backup_node(s, false, true) < 0) { status = MP_ERR_ARG; break; }
                const double top = amax_listed(s, 0);
                const int a = draw_tie_chunks(A, [&](int b) { return listed(s, b) && c_val[2 * ((long)s * A + b)] == top; }, gen);
                // the clone's step: `done` is discarded (:251)
                const long sa = (long)s * A + a;
                int sn;
                double rew;
                if (table) {
                    const Rec rc = p.rec[sa];
                    sn = rc.next; rew = rc.reward;
                } else {
                    const uint64_t u = eg.next64() >> 11;          // Generator.random() of the clone's generator
                    const uint64_t *trow = p.thr + sa * p.W;
                    int lo = 0;                                    // searchsorted(cdf, u, 'right') = #{j : thr_j <= u}
                    for (int j0 = 0; j0 < p.W; j0 += 64) {
                        const int jj = j0 + lane;
                        const unsigned long long bal = ballot64(jj < p.W && trow[jj] <= u);
                        lo += __popcll(bal);
                        if (bal != ~0ull) break;
                    }
                    if (lo >= p.W) lo = p.W - 1;
                    sn = p.mode == MP_MODE_SPARSE ? p.nxt[sa * p.W + lo] : lo;
                    rew = p.R[sa];
                }
                sn = __builtin_amdgcn_readfirstlane(sn);
                if ((unsigned)sn >= (unsigned)S) { status = MP_ERR_ARG; break; } // (never follow a record outside the tables)
                ++steps;
                if (l0) visits[sn] += 1; // planner.step, abstract.py:158-161
                // GraphChanceNode.get_child (:207-219)
                const int m = c_m[sa];
                const unsigned long long hit = ballot64(lane < m && k_state[sa * K + lane] == sn);
                int j;
                if (hit) j = __ffsll((long long)hit) - 1;
                else if (m < K) {
                    j = m;
                    if (l0) { k_state[sa * K + m] = sn; c_m[sa] = m + 1; }
                    get_node(sn);
                    // parents.add(self.parent): a set
                    const int base = p.in_ptr[sn], room = p.in_ptr[sn + 1] - base;
                    int np_ = npar[sn];
                    if (np_ > room) np_ = room;
                    bool found = false;
                    for (int j0 = 0; j0 < np_; j0 += 64) found = any64(j0 + lane < np_ && par[base + j0 + lane] == s) || found;
                    if (!found) {
                        if (np_ >= room) { status = MP_ERR_ARG; break; } // (tables changed under a kept graph: never write past the slice)
                        if (l0) { par[base + np_] = s; npar[sn] = np_ + 1; }
                    }
                } else { status = MP_ERR_GBOP_PLACEHOLDERS; break; } // :217-218, after the step was counted
                // update (:62-66, :164-165)
                const long kj = sa * K + j;
                const int kc = k_count[kj] + 1;
                const double cum = k_cum[kj] + rew;
                if (l0) { count[s] += 1; c_count[sa] += 1; k_count[kj] = kc; k_cum[kj] = cum; }
                if (kc > p.n_counts) { status = MP_ERR_ARG; break; }
                // compute_reward_ucb (:68-82): a threshold other than 0 reaches the mis-called kl_upper_bound
                if (p.rthr[kc - 1] != 0.0) { status = MP_ERR_GBOP_REWARD_THRESHOLD; break; }
                if (l0) { const double mu = cum / (double)kc; k_mu[kj] = mu; k_lcb[kj] = mu; }
                // update_queue (:264-265)
                bool queued = false;
                for (int j0 = 0; j0 < nq; j0 += 64) queued = any64(j0 + lane < nq && uq[j0 + lane] == s) || queued;
                if (!queued) {
                    if (l0) uq[nq] = s; // (nq < S: the entries are distinct states)
                    ++nq;
                }
                s = sn;
                __syncthreads();
            }
            if (status != MP_OK) break;
            // ---- partial_value_iteration(queue=reversed(update_queue)), :89-101
            if (nq > p.qcap) { status = MP_ERR_ALLOC; break; }
            for (int i = lane; i < nq; i += 64) queue[i] = uq[nq - 1 - i];
            unsigned qh = 0, qt = (unsigned)nq;
            __syncthreads();
            while (qh != qt) {
                const int v = __builtin_amdgcn_readfirstlane(queue[qh & qmask]);
                if (pops_total >= p.max_pops) { status = MP_ERR_GBOPD_DIVERGED; break; } // (the front stays unpopped)
                ++qh; ++pops_total;
                const double old_l = lower[v], old_u = upper[v];
                if (backup_node(v, true, true) < 0) { status = MP_ERR_ARG; break; }
                const double bl = amax_listed(v, 1), bu = amax_listed(v, 0);
                double delta = 0.0;
                const double dl = fabs(old_l - bl), du = fabs(old_u - bu);
                if (dl > delta) delta = dl;
                if (du > delta) delta = du;
                if (l0) { lower[v] = bl; upper[v] = bu; }
                if (delta > p.accuracy) { // queue.extend(list(node.parents)), insertion order
                    const int base = p.in_ptr[v], room = p.in_ptr[v + 1] - base;
                    int np_ = npar[v];
                    if (np_ > room) np_ = room;
                    if (qt - qh + (unsigned)np_ > (unsigned)p.qcap) { status = MP_ERR_ALLOC; break; }
                    for (int j = lane; j < np_; j += 64) queue[(qt + (unsigned)j) & qmask] = par[base + j];
                    qt += (unsigned)np_;
                }
                __syncthreads();
            }
        }
        // ---- get_plan (graph_based.py:126-135): the root's selection_rule (:53-60), then the chosen chance node's (:152-156)
        int len = 0, action = -1, key = 0;
        if (status == MP_OK && p.plan_steps >= 1 && expanded[s0]) {
            __syncthreads();
            if (backup_node(s0, false, false) < 0) status = MP_ERR_ARG;
            else {
                const double top = amax_listed(s0, 1);
                action = draw_tie_chunks(A, [&](int b) { return listed(s0, b) && c_val[2 * ((long)s0 * A + b) + 1] == top; }, gen);
                len = 1;
            }
            if (status == MP_OK && p.plan_steps >= 2) {
                // Generator.choice(keys, p=p_minus): the checks of p (Kahan sum within sqrt(eps) of 1), cdf = cumsum / cdf[-1],
                // one double, searchsorted(side="right").  K <= 32 entries, uniform code.
                const long sa = (long)s0 * A + action;
                const double *pmin = pm + sa * K;
                double sum = pmin[0], comp = 0.0, total = 0.0;
                bool bad = pmin[0] < 0.0;
                for (int i = 0; i < K; ++i) {
                    const double v = pmin[i];
                    if (i > 0) {
                        const double y = v - comp, t = sum + y;
                        comp = (t - sum) - y;
                        sum = t;
                        bad = bad || v < 0.0;
                    }
                    total += v;
                }
                if (!(fabs(sum - 1.0) <= 1.4901161193847656e-08) || bad) status = MP_ERR_GBOP_CHOICE_P; // (NaN included)
                else {
                    const double u = gen.next_double();
                    double c = 0.0;
                    int idx = 0;
                    for (int i = 0; i < K; ++i) {
                        c += pmin[i];
                        if (c / total <= u) ++idx;
                    }
                    if (idx >= K) idx = K - 1; // (cdf[-1] = 1 > u: not reached)
                    key = k_state[sa * K + (idx + c_m[sa]) % K];
                    len = 2;
                }
            }
            if (status != MP_OK) { len = 0; action = -1; key = 0; }
        }
        const double root_l = lower[s0], root_u = upper[s0];
        if (LDSV) graph_write_back(p.lower, p.upper, sb, created, n_created, lower, upper, lane);
        if (l0) {
            gen.store(p.rng + (long)r * 6);
            p.n_created[r] = n_created;
            p.n_obs[r] += steps;
            if (status != MP_OK) p.failed[r] = status; // sticky: the graph is half updated
            if (p.action) p.action[r] = action;
            if (p.key) p.key[r] = key;
            if (p.plan_len) p.plan_len[r] = len;
            if (p.status) p.status[r] = status;
            if (p.root_lower) p.root_lower[r] = root_l;
            if (p.root_upper) p.root_upper[r] = root_u;
            if (p.env_steps) p.env_steps[r] = steps;
            if (p.pops) p.pops[r] = pops_total;
        }
    }
}

} // namespace mp

using namespace mp;

extern "C" {

int mp_gbop_free(mp_gbop *pl) { return graph_free(pl); }

int mp_gbop_create(mp_ctx *ctx, mp_model *model, int32_t n_planners, int32_t max_next_states, int32_t queue_cap, mp_gbop **out)
{
    const char *const who = "mp_gbop_create";
    if (!ctx || !model || !out) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    MP_TRY(wave_mdp_check(who, model, false));
    const int K = max_next_states;
    if (K < 1 || K > 32)
        return fail(MP_ERR_ARG, "%s: max_next_states_count %d is not in 1..32 (a chance node's children fill half a wavefront)", who, K);
    if (n_planners < 1 || model->S < 1 || model->A < 1) return fail(MP_ERR_ARG, "%s: n_planners = %d", who, n_planners);
    MP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (model->mode != MP_MODE_DETERMINISTIC) MP_TRY(ensure_thresholds(ctx, who, model));
    mp_gbop *pl = new (std::nothrow) mp_gbop;
    if (!pl) return fail(MP_ERR_ALLOC, "%s: out of memory", who);
    pl->ctx = ctx; pl->model = model; pl->model_serial = model->serial; pl->n = n_planners; pl->S = model->S; pl->A = model->A; pl->K = K;
    const int S = pl->S, A = pl->A;
    const size_t SA = (size_t)S * A;
    // (an episode's update_queue holds distinct states: a ring of fewer than S entries can fail on its first episode)
    const int q = pl->qcap = graph_queue_capacity(queue_cap, "MP_GBOP_QUEUE", n_planners);
    // the listed actions and the in-degrees on the host: the distinct states with a listed action that may lead to c
    const int W = model->mode == MP_MODE_DETERMINISTIC ? 1 : model->mode == MP_MODE_STOCHASTIC ? S : model->B;
    std::vector<Rec> hrec;
    std::vector<uint64_t> hthr;
    std::vector<int32_t> hnxt;
    std::vector<uint8_t> havail;
    hipError_t e = hipStreamSynchronize(st);
    if (model->mode == MP_MODE_DETERMINISTIC) {
        hrec.resize(SA);
        if (e == hipSuccess) e = hipMemcpy(hrec.data(), model->rec, SA * sizeof(Rec), hipMemcpyDeviceToHost);
    } else {
        hthr.resize(SA * W);
        if (e == hipSuccess) e = hipMemcpy(hthr.data(), model->thr, SA * W * sizeof(uint64_t), hipMemcpyDeviceToHost);
        if (model->mode == MP_MODE_SPARSE) {
            hnxt.resize(SA * W);
            if (e == hipSuccess) e = hipMemcpy(hnxt.data(), model->NXT, SA * W * sizeof(int32_t), hipMemcpyDeviceToHost);
        }
        if (model->masked && model->avail) {
            havail.resize(SA);
            if (e == hipSuccess) e = hipMemcpy(havail.data(), model->avail, SA, hipMemcpyDeviceToHost);
        }
    }
    if (e != hipSuccess) {
        delete pl;
        return fail(MP_ERR_HIP, "%s: reading the model's tables failed", who);
    }
    pl->h_listed.assign(SA, 0);
    const int counted = graph_count_parents(pl, who, [&](int s, int a, auto visit) {
        const size_t sa = (size_t)s * A + a;
        const bool is_listed = model->mode == MP_MODE_DETERMINISTIC ? (hrec[sa].flags & 4u) != 0 : (havail.empty() || havail[sa] != 0);
        pl->h_listed[sa] = is_listed ? 1 : 0;
        if (!is_listed) return (int)MP_OK;
        if (model->mode == MP_MODE_DETERMINISTIC) return visit(hrec[sa].next);
        for (int j = 0; j < W; ++j) {
            // the row search can return column j only where its threshold exceeds the one before; the last column also
            // takes a draw past every threshold
            const uint64_t before = j ? hthr[sa * W + j - 1] : 0;
            if (!(hthr[sa * W + j] > before) && j != W - 1) continue;
            MP_TRY(visit(model->mode == MP_MODE_SPARSE ? hnxt[sa * W + j] : j));
        }
        return (int)MP_OK;
    });
    if (counted != MP_OK) {
        delete pl;
        return counted;
    }
    const size_t sn = (size_t)S * pl->n, cn = sn * A, kn = cn * K;
    int made = graph_create_shared(pl);
    if (made == MP_OK &&
        (graph_alloc(pl, &pl->uq, sn * 4) != hipSuccess || graph_alloc(pl, &pl->count, sn * 8) != hipSuccess ||
         graph_alloc(pl, &pl->c_count, cn * 4) != hipSuccess || graph_alloc(pl, &pl->c_m, cn * 4) != hipSuccess ||
         graph_alloc(pl, &pl->c_backed, cn * 4) != hipSuccess || graph_alloc(pl, &pl->c_val, cn * 16) != hipSuccess ||
         graph_alloc(pl, &pl->k_state, kn * 4) != hipSuccess || graph_alloc(pl, &pl->k_count, kn * 4) != hipSuccess ||
         graph_alloc(pl, &pl->k_cum, kn * 8) != hipSuccess || graph_alloc(pl, &pl->k_mu, kn * 8) != hipSuccess ||
         graph_alloc(pl, &pl->k_lcb, kn * 8) != hipSuccess || graph_alloc(pl, &pl->pp, kn * 8) != hipSuccess ||
         graph_alloc(pl, &pl->pm, kn * 8) != hipSuccess))
        made = MP_ERR_ALLOC;
    // (the chance records of a state are initialised when it is expanded)
    if (made == MP_OK && (hipMemsetAsync(pl->count, 0, sn * 8, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) made = MP_ERR_HIP;
    if (made != MP_OK) {
        (void)hipGetLastError();
        mp_gbop_free(pl);
        if (made == MP_ERR_HIP) return fail(MP_ERR_HIP, "%s: initialising the planners failed", who);
        return fail(MP_ERR_ALLOC, "%s: device allocation failed (%d planners x %d states x %d actions x %d next states, queue of %d "
                                  "entries each)", who, n_planners, S, A, K, q);
    }
    *out = pl;
    return MP_OK;
}

int mp_gbop_plan(mp_ctx *ctx, mp_gbop *pl, const int32_t *root_state, int32_t episodes, int32_t horizon, int32_t max_next_states,
                 double gamma, double value_max, double accuracy, int32_t sampling_timeout, int32_t n_counts,
                 const double *reward_thr_by_count, const double *transition_thr_by_count, uint64_t *rng_state, int32_t *action,
                 int32_t *key, int32_t *plan_len, double *value_lower, double *value_upper, int64_t *env_steps, int64_t *pops,
                 int32_t *status, int32_t mem)
{
    const char *const who = "mp_gbop_plan";
    if (!ctx || !pl || !root_state || !rng_state || !reward_thr_by_count || !transition_thr_by_count)
        return fail(MP_ERR_ARG, "%s: NULL argument", who);
    int rmem;
    MP_TRY(wave_mem(who, &mem, &rmem));
    MP_TRY(graph_check_handle(ctx, pl, who, "bounds, parents, counts and chance records"));
    if (max_next_states < 1 || max_next_states > 32)
        return fail(MP_ERR_ARG, "%s: max_next_states_count %d is not in 1..32", who, max_next_states);
    if (max_next_states != pl->K)
        return fail(MP_ERR_ARG, "%s: max_next_states_count %d, but the planners' chance records hold %d children", who,
                    max_next_states, pl->K);
    if (episodes < 0 || horizon < 1 || sampling_timeout < 0) // (horizon 0: the reference's run() raises UnboundLocalError)
        return fail(MP_ERR_ARG, "%s: episodes = %d, horizon = %d, sampling_timeout = %d", who, episodes, horizon, sampling_timeout);
    MP_TRY(graph_check_numbers(who, gamma, value_max, accuracy));
    // counts are LIFETIME counts: none exceeds the steps made so far plus this call's
    const int64_t reach = pl->steps_bound + (int64_t)episodes * horizon;
    if (reach > 0x7fffffff) return fail(MP_ERR_ARG, "%s: %lld lifetime steps do not fit a 32-bit count", who, (long long)reach);
    if ((int64_t)n_counts < reach)
        return fail(MP_ERR_ARG, "%s: the threshold tables hold %d counts, %lld are reachable by the end of this call", who, n_counts,
                    (long long)reach);
    for (int64_t c = 0; c < reach; ++c)
        if (!isfinite(reward_thr_by_count[c]) || !isfinite(transition_thr_by_count[c]))
            return fail(MP_ERR_ARG, "%s: a threshold of count %lld is not finite", who, (long long)c + 1);
    const int n = pl->n, S = pl->S;
    MP_TRY(wave_roots(ctx, who, root_state, n, S, mem));

    GbopArgs a;
    MP_TRY(wave_mdp(ctx, who, pl->model, &a));
    std::vector<double> tab(2 * (size_t)reach + 2);
    for (int64_t c = 0; c < reach; ++c) { tab[c] = reward_thr_by_count[c]; tab[reach + c] = transition_thr_by_count[c]; }
    double *d_tab = nullptr;
    MP_TRY(upload_tables(ctx, 44, tab, &d_tab));
    graph_args(pl, "MP_GBOP_MAX_POPS", gamma, value_max, accuracy, &a);
    a.K = pl->K; a.M = episodes; a.H = horizon;
    a.plan_steps = sampling_timeout < 2 ? sampling_timeout : 2; a.n_counts = (int)reach;
    a.avail = pl->model->masked ? pl->model->avail : nullptr;
    a.rthr = d_tab; a.tthr = d_tab + reach;
    a.c_val = pl->c_val; a.k_cum = pl->k_cum; a.k_mu = pl->k_mu; a.k_lcb = pl->k_lcb; a.pp = pl->pp; a.pm = pl->pm;
    a.uq = pl->uq; a.c_count = pl->c_count; a.c_m = pl->c_m; a.c_backed = pl->c_backed; a.k_state = pl->k_state; a.k_count = pl->k_count;
    a.count = pl->count;
    WaveIo io(mem, rmem, n, root_state, &a.root_state, rng_state, &a.rng);
    io.add(WS_IO3, action, &a.action);
    graph_results_io(io, plan_len, status, env_steps, pops, value_lower, value_upper, &a);
    io.add(WS_IO1, key, &a.key);
    MP_TRY(wave_stage(ctx, io));

    // both bounds in LDS while they are small; MP_GBOP_LDS_BYTES moves the limit
    const bool use_lds = graph_use_lds("MP_GBOP_LDS_BYTES", S);
    // the workgroups stride over the planners: 16 wavefronts a compute unit; MP_GBOP_GRID lowers the grid (tests)
    long grid = (long)ctx->prop.multiProcessorCount * 16;
    if (const char *e = getenv("MP_GBOP_GRID")) {
        const long v = atol(e);
        if (v >= 1 && v < grid) grid = v;
    }
    if (grid > n) grid = n;
    pl->steps_bound = reach;
    MP_TRY(wave_launch(ctx, use_lds ? gbop_kernel<true> : gbop_kernel<false>, (int)grid, use_lds ? (size_t)S * 16 : 0,
                       gbop_form_name(pl->model->mode, use_lds), a));
    return wave_unstage(ctx, io);
}

const char *mp_gbop_form_names(void)
{
    static const std::string names = gbop_form_names();
    return names.c_str();
}

int mp_gbop_info(mp_gbop *pl, int32_t *n_planners, int32_t *n_states, int32_t *n_actions, int32_t *max_next_states,
                 int32_t *queue_cap, int64_t *n_edges, int64_t *max_count)
{
    if (!pl) return fail(MP_ERR_ARG, "mp_gbop_info: planner is NULL");
    if (n_planners) *n_planners = pl->n;
    if (n_states) *n_states = pl->S;
    if (n_actions) *n_actions = pl->A;
    if (max_next_states) *max_next_states = pl->K;
    if (queue_cap) *queue_cap = pl->qcap;
    if (n_edges) *n_edges = pl->E;
    if (max_count) *max_count = pl->steps_bound;
    return MP_OK;
}

int mp_gbop_export(mp_gbop *pl, int32_t planner, int32_t cap, int32_t *n_nodes, int32_t *state, double *lower, double *upper,
                   uint8_t *expanded, int64_t *count, uint8_t *listed, int32_t *chance_count, int32_t *chance_assigned,
                   int32_t *chance_backed, double *chance_value, int32_t *child_state, int32_t *child_count,
                   double *child_cumulative_reward, double *child_mu_ucb, double *child_mu_lcb, double *p_plus, double *p_minus,
                   int32_t *parent_ptr, int32_t *parent_idx, int64_t *visits, int64_t *n_observations, int32_t *root)
{
    const char *const who = "mp_gbop_export";
    GraphExport x;
    MP_TRY(graph_export_begin(pl, who, "actions", planner, cap, n_nodes, visits, n_observations, root, &x));
    const size_t S = (size_t)pl->S, A = (size_t)pl->A, K = (size_t)pl->K, r = (size_t)planner, SA = S * A, SAK = SA * K;
    std::vector<double> hcv(2 * SA), hcum(SAK), hmu(SAK), hlcb(SAK), hpp(SAK), hpm(SAK);
    std::vector<int32_t> hcc(SA), hcm(SA), hcb(SA), hks(SAK), hkc(SAK);
    std::vector<int64_t> hcount(S);
    MP_HIP(hipMemcpy(hcount.data(), pl->count + r * S, S * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hcc.data(), pl->c_count + r * SA, SA * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hcm.data(), pl->c_m + r * SA, SA * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hcb.data(), pl->c_backed + r * SA, SA * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hcv.data(), pl->c_val + r * 2 * SA, 2 * SA * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hks.data(), pl->k_state + r * SAK, SAK * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hkc.data(), pl->k_count + r * SAK, SAK * 4, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hcum.data(), pl->k_cum + r * SAK, SAK * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hmu.data(), pl->k_mu + r * SAK, SAK * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hlcb.data(), pl->k_lcb + r * SAK, SAK * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hpp.data(), pl->pp + r * SAK, SAK * 8, hipMemcpyDeviceToHost));
    MP_HIP(hipMemcpy(hpm.data(), pl->pm + r * SAK, SAK * 8, hipMemcpyDeviceToHost));
    int32_t np_total = 0;
    if (parent_ptr) parent_ptr[0] = 0;
    for (int32_t i = 0; i < x.n_nodes; ++i) {
        const int32_t s = x.created[(size_t)i];
        if (s < 0 || (size_t)s >= S) return fail(MP_ERR_ARG, "%s: node %d holds state %d", who, i, s);
        if (state) state[i] = s;
        if (lower) lower[i] = x.lower[(size_t)s];
        if (upper) upper[i] = x.upper[(size_t)s];
        if (expanded) expanded[i] = x.expanded[(size_t)s];
        if (count) count[i] = hcount[(size_t)s];
        for (size_t a = 0; a < A; ++a) { // the chance records by action slot (slot = listing order); zeros where there is none
            const size_t src = (size_t)s * A + a, dst = (size_t)i * A + a;
            const bool has = x.expanded[(size_t)s] && pl->h_listed[src];
            if (listed) listed[dst] = has ? 1 : 0;
            if (chance_count) chance_count[dst] = has ? hcc[src] : 0;
            if (chance_assigned) chance_assigned[dst] = has ? hcm[src] : 0;
            if (chance_backed) chance_backed[dst] = has ? hcb[src] : -1;
            if (chance_value) { chance_value[2 * dst] = has ? hcv[2 * src] : 0.0; chance_value[2 * dst + 1] = has ? hcv[2 * src + 1] : 0.0; }
            for (size_t k = 0; k < K; ++k) {
                const size_t ks = src * K + k, kd = dst * K + k;
                if (child_state) child_state[kd] = has ? hks[ks] : 0;
                if (child_count) child_count[kd] = has ? hkc[ks] : 0;
                if (child_cumulative_reward) child_cumulative_reward[kd] = has ? hcum[ks] : 0.0;
                if (child_mu_ucb) child_mu_ucb[kd] = has ? hmu[ks] : 0.0;
                if (child_mu_lcb) child_mu_lcb[kd] = has ? hlcb[ks] : 0.0;
                if (p_plus) p_plus[kd] = has ? hpp[ks] : 0.0;
                if (p_minus) p_minus[kd] = has ? hpm[ks] : 0.0;
            }
        }
        graph_export_parents(pl, x, i, s, parent_ptr, parent_idx, &np_total);
    }
    return MP_OK;
}

} // extern "C"
