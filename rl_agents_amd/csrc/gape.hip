// gape.hip -- MDP-GapE, best-arm identification at the root of a tree of decision and chance nodes (tree_search/mdp_gape.py,
// olop.py:132-142, utils.py:89-203), on deterministic tables with one next state per chance node (max_next_states_count 1).
//
// Mapping: ONE ROOT PER WAVEFRONT (one 64-lane workgroup), the workgroups striding over the roots, as olop.hip.  A plan is at most
// `episodes + 2` episodes (mdp_gape.py:94-110) of exactly `horizon` model steps:
//   * the walk is the serial chain, one model step per depth, every lane holding the same (wave-uniform) state and generator;
//   * the lanes cover a node's chance children, 64 at a time when |A| > 64: their creation at an expansion (one 16-byte model
//     gather each, listing order by a ballot prefix count), the root's best-arm identification (:228-249: gaps, first minimum,
//     challenger, the wider of the two), the tie set of random_argmax over value_upper below the root (:189-192, exact equality,
//     a draw only for two or more ties) and the backup's two np.amax (:219-220);
//   * the 2 * horizon Newton solves of an episode's path -- mu_ucb and mu_lcb of every decision node stepped into -- are
//     independent (a node is on the path once and only the backup reads them): they go on the lanes after the walk, 64 at a time.
// With one next state, p_hat = [1.0] and max_expectation_under_constraint returns it (utils.py:325-326), so a chance node's
// values are mu + gamma * value of its decision child (:296-304), both sides.
// A chance node and its single decision child share ONE record (GapeNode): the chance node's two values sit in a second array,
// [cap][2], which is what the lanes read; the record keeps the order in which the two were created (cseq, dseq) for the export.
// Records live in the wave_tree workspace, children contiguous in creation order: at most 1 + (episodes + 2) * horizon * |A|.
// Everything that is not a basic IEEE operation -- the initial values (Python **), the thresholds by count (eval of the config
// string) -- comes from host tables.  The Newton step's log is the device's (bounds to 1e-12, not bit-exact).
// What this file has in common with gape_stoch.hip -- the result arrays, the argument checks, the capacity refusals and the tables
// of the host side; the stopping rule and the read-out of a root on the device -- is in gape_shared.hpp, the selection among a
// node's children in gape_select.hpp.  The episode loop, the listing of an expansion and the deferred bounds included, is here.
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
#include "wave.hpp"

namespace mp {

struct GapeNode {
    double cum, mu_ucb, mu_lcb;     // the decision child: cumulative_reward, mu_ucb, mu_lcb (olop.py:109-116, mdp_gape.py:139-143)
    double vu, vl;                  // the decision child's value_upper / value_lower
    int32_t count_c, count_d;       // visits of the chance node and of its decision child (equal once stepped through)
    int32_t state, parent, first_child, n_children; // the child's state; the record of the parent decision node; the child's children
    int32_t action, depth, done;    // the chance node's action (a column); the CHILD's depth (the chance node's is depth - 1)
    int32_t cseq, dseq, pad;        // creation numbers of the chance node and of the decision child (-1: not created yet)
};
static_assert(sizeof(GapeNode) == 88, "GapeNode layout");

struct GapeArgs {
    int n_roots, A, M, H, cap, done_on_next, uniform, n_env, keep, grid, max_plan_len;
    int Sb;              // states of one MDP of a batch model (mp_gape_plan_models), else |S|
    double gamma, accuracy;
    const Rec *rec;
    const int32_t *root_state;
    const double *thr;   // [M + 2] threshold by count - 1
    const double *vinit; // [H + 1] (1 - gamma ** (H - d)) / (1 - gamma)
    const double *col;   // [n_env] the column of environment action a, -1 without one (small integers, kept in the double table)
    uint64_t *rng;
    GapeNode *nodes;     // [slots][cap]
    double *val;         // [slots][cap][2] the chance nodes' value_upper, value_lower
    int32_t *n_nodes_out;
    GapeResults out;
};

// EACH (mp_gape_plan_models: a batch model of deterministic tables, one MDP per root, the roots' states GLOBAL -- nodes keep
// global states, and the availability flag and the done bits are those of the global state's records).  GAPE_WHOLE is the kernel
// of mp_gape_plan; GAPE_EACH_GLOBAL is the same code on the batch model's records; GAPE_EACH_LDS copies the root's own Sb * |A|
// records into LDS behind path[] -- before its first episode, and again only when a workgroup's next root sits on another MDP --
// and serves both kinds of model read, the expansion's row and the step's record, from there: a record's `next` lies inside
// the root's MDP (mp_model_load_table_batch checks it), so its index is (state - base) * |A| + a.  Everything the LDS form adds
// sits under `if constexpr` (profiles/gape_each_kernel_resources.txt).
enum { GAPE_WHOLE = 0, GAPE_EACH_GLOBAL = 1, GAPE_EACH_LDS = 2 };

template <int EACH>
__global__ __launch_bounds__(64) void gape_kernel(GapeArgs p)
{
    extern __shared__ int32_t path[]; // [H + 1] records of the episode's walk
    const int lane = threadIdx.x, A = p.A, H = p.H;
    constexpr bool lds_model = EACH == GAPE_EACH_LDS;
    Rec *lrec = nullptr;              // [Sb * A] GAPE_EACH_LDS: the root's table, 16-byte aligned behind path[]
    if constexpr (lds_model) lrec = static_cast<Rec *>(__builtin_assume_aligned(path + ((H + 1 + 3) & ~3), 16));
    int base = 0, loaded = -1;        // GAPE_EACH_LDS: first global state of the root's MDP / index of the MDP in LDS
    // the records of state `s` (GLOBAL), one per action
    auto row_of = [&](int s) -> const Rec * { return lds_model ? lrec + (long)(s - base) * A : p.rec + (long)s * A; };
    const uint32_t done_bit = p.done_on_next ? 2u : 1u;
    for (int root = blockIdx.x; root < p.n_roots; root += p.grid) {
        const long slot = p.keep ? root : (root == 0 ? p.grid : blockIdx.x);
        GapeNode *N = p.nodes + slot * p.cap;
        double *V = p.val + slot * p.cap * 2;
        // GAPE_EACH_LDS: the root's table into LDS (the previous root's reads ended at the barrier that closes its iteration; this
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
            GapeNode r;
            r.cum = 0.0; r.mu_ucb = 1.0; r.mu_lcb = 0.0; r.vu = p.vinit[0]; r.vl = 0.0; r.count_c = 0; r.count_d = 0;
            r.state = p.root_state[root]; r.parent = -1; r.first_child = -1; r.n_children = 0; r.action = -1; r.depth = 0; r.done = 0;
            r.cseq = -1; r.dseq = 0; r.pad = 0;
            N[0] = r;
            V[0] = 0.0; V[1] = 0.0;
        }
        __syncthreads();
        Pcg64 gen;
        gen.load(p.rng + (long)root * 6);
        int n_nodes = 1, n_created = 1, status = MP_OK, episodes_run = 0, best = -1, challenger = -1;
        long steps = 0;

        // DecisionNode.expand (mdp_gape.py:162-170): a chance child per listed action, in listing order; *rank = the position
        // of column `col` among them, -1 when it is not listed
        auto expand = [&](int node, int state, int depth, int col, int *rank) {
            const Rec *row = row_of(state);
            const int fc = n_nodes;
            int pos0 = 0;
            *rank = -1;
            for (int a0 = 0; a0 < A; a0 += 64) {
                const int a = a0 + lane;
                Rec rc;
                bool av = false;
                if (a < A) { rc = row[a]; av = (rc.flags & 4u) != 0; }
                const unsigned long long bal = __ballot(av);
                const int pos = pos0 + __popcll(bal & ((1ull << lane) - 1ull));
                if (av) {
                    GapeNode c;
                    c.cum = 0.0; c.mu_ucb = 1.0; c.mu_lcb = 0.0; c.vu = p.vinit[depth + 1]; c.vl = 0.0; c.count_c = 0; c.count_d = 0;
                    c.state = rc.next; c.parent = node; c.first_child = -1; c.n_children = 0; c.action = a; c.depth = depth + 1;
                    c.done = 0; c.cseq = n_created + pos; c.dseq = -1; c.pad = 0;
                    N[fc + pos] = c;
                    V[2 * (fc + pos)] = p.vinit[depth]; // a chance node has its parent's depth (mdp_gape.py:256-258)
                    V[2 * (fc + pos) + 1] = 0.0;
                }
                if (col >= a0 && col < a0 + 64 && ((bal >> (col - a0)) & 1ull))
                    *rank = pos0 + __popcll(bal & ((1ull << (col - a0)) - 1ull));
                pos0 += __popcll(bal);
            }
            if (lane == 0) { N[node].first_child = fc; N[node].n_children = pos0; }
            n_nodes += pos0;
            n_created += pos0;
            __syncthreads();
            return pos0;
        };

        for (int e = 0; e < p.M + 2 && status == MP_OK; ++e) {
            gen.below(1u << 30); // state.seed(self.np_random.randint(2**30)), mdp_gape.py:67
            if (N[0].n_children == 0) {
                int unused;
                expand(0, N[0].state, 0, -1, &unused);
            }
            int node = 0;
            if (lane == 0) path[0] = 0;
            for (int h = 0; h < H; ++h) {
                const GapeNode nd = N[node];
                int fc = nd.first_child, k = nd.n_children, j;
                if (node == 0) { // sampling_rule at the root: the arm best-arm identification selects (mdp_gape.py:185-187)
                    // one listed action: max() of an empty list (:247).  (None at all cannot be: mp_model_set_available
                    // asks for one in every state; the reference would fail in min() there.)
                    if (k < 2) { status = MP_ERR_GAPE_NO_CHALLENGER; break; }
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
                    k = expand(node, nd.state, nd.depth, col, &rank);
                    j = rank >= 0 ? rank : 0;
                }
                const int child = fc + j;
                const GapeNode c0 = N[child];
                const Rec rc = row_of(nd.state)[c0.action];
                ++steps;
                const double r = rc.reward;
                // olop.py:133-134, after the step was counted.  (The reference has also counted the chance node and made its
                // decision child by then; the tree of a failed plan is not kept in that state: nothing reads it.)
                if (!(0.0 <= r && r <= 1.0)) { status = MP_ERR_REWARD_RANGE; break; }
                if (lane == 0) { // ChanceNode.update (:264-265), get_child (:272-286), OLOPNode.update (olop.py:132-142)
                    GapeNode c = c0;
                    c.count_c += 1;
                    if (c.dseq < 0) c.dseq = n_created;
                    if (rc.flags & done_bit) c.done = 1;
                    c.cum += c.done ? 0.0 : r;
                    c.count_d += 1;
                    N[child] = c;
                    path[h + 1] = child;
                }
                if (c0.dseq < 0) ++n_created;
                node = child;
                __syncthreads();
            }
            if (status != MP_OK) break;
            // compute_reward_ucb (mdp_gape.py:200-210) of the path's decision nodes: H upper bounds, then H lower bounds
            for (int t0 = 0; t0 < 2 * H; t0 += 64) {
                const int t = t0 + lane;
                if (t < 2 * H) {
                    const bool lower = t >= H;
                    GapeNode *c = N + path[1 + (lower ? t - H : t)];
                    const double thr = p.thr[c->count_d - 1];
                    if (lower) c->mu_lcb = kl_upper_bound<false, true>(c->cum, c->count_d, thr);
                    else c->mu_ucb = kl_upper_bound<false, false>(c->cum, c->count_d, thr);
                }
            }
            __syncthreads();
            // backup_to_root (:214-226, :288-305), from the depth-H decision node up
            for (int h = H; h >= 0; --h) {
                const int id = path[h];
                const GapeNode nd = N[id];
                double vu = 0.0, vl = 0.0; // the depth-H node has no children
                if (nd.n_children > 0) {
                    vu = gape_amax(V + 2 * (long)nd.first_child, nd.n_children, 0, lane);
                    vl = gape_amax(V + 2 * (long)nd.first_child, nd.n_children, 1, lane);
                }
                if (lane == 0) {
                    N[id].vu = vu; N[id].vl = vl;
                    if (h > 0) {
                        V[2 * (long)id] = nd.mu_ucb + p.gamma * vu;
                        V[2 * (long)id + 1] = nd.mu_lcb + p.gamma * vl;
                    }
                }
                __syncthreads();
            }
            episodes_run = e + 1;
            if (gape_stop(V, N[0].first_child, N[0].n_children, lane, p.accuracy, &best, &challenger)) break;
        }
        const int fc0 = N[0].first_child;
        gape_read_out(p.out, p.rng, root, A, p.max_plan_len, lane, V, fc0, N[0].n_children, gen, status, best, challenger, episodes_run,
                      steps, [&](int i) { return N[fc0 + i].action; }, [&](int i) { return N[fc0 + i].count_c; });
        if (lane == 0) p.n_nodes_out[root] = n_nodes;
        __syncthreads();
    }
}

inline FormName gape_form_name(bool keep) { return slots_form_name("gape", keep); }
// mp_gape_plan_models: the root's table in LDS or read from global memory, with the `_slots` suffix of slots_form_name.  Listed by
// mp_gape_each_form_names, part of no other list of names.
inline FormName gape_each_form_name(bool lds, bool keep)
{
    if (!lds) return slots_form_name("gape_each", keep);
    FormName n;
    snprintf(n.s, sizeof(n.s), "gape_each_lds%s", keep ? "" : "_slots");
    return n;
}

} // namespace mp

using namespace mp;

extern "C" {

extern "C++" {
namespace {
// mp_gape_plan (model_index NULL: `root_state` holds states of the one table) and mp_gape_plan_models (a batch model of
// deterministic tables, `root_state` LOCAL to the MDP model_index names: globalize_roots_arg makes the GLOBAL states the kernel
// plans from, and the form is each_form's)
int gape_plan_impl(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                   int32_t episodes, int32_t horizon, double gamma, double accuracy, int32_t continuation, int32_t n_actions_env,
                   const int32_t *action_column, const double *thr_by_count, const double *value_init, uint64_t *rng_state,
                   int32_t max_plan_len, int32_t *plans, int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps,
                   int32_t *status, double *child_lower, double *child_upper, int64_t *child_count, int32_t *best_challenger,
                   int32_t mem, bool each)
{
    const char *const who = each ? "mp_gape_plan_models" : "mp_gape_plan";
    if (!ctx || !model || !root_state || !rng_state || !thr_by_count || !value_init || (each && !model_index))
        return fail(MP_ERR_ARG, "%s: NULL argument", who);
    const int32_t mem_flags = mem;
    int rmem;
    MP_TRY(wave_mem(who, &mem, &rmem));
    if (model->mode != MP_MODE_DETERMINISTIC)
        return fail(MP_ERR_MODE, "%s: model mode %d is not a deterministic table (a dense or sparse model needs the reference's "
                                 "transition bounds, which are not built)", who, model->mode);
    MP_TRY(wave_mdp_check(who, model, each));
    if (each && !model->table_batch)
        return fail(MP_ERR_MODE, "%s: a batch model of deterministic tables (mp_model_load_table_batch) expected", who);
    const int A = model->A;
    const GapeTables host_tab{thr_by_count, nullptr, value_init, nullptr};
    MP_TRY(gape_check_args(who, n_roots, episodes, horizon, 16384, max_plan_len, A, n_actions_env, gamma, accuracy, host_tab,
                           continuation, action_column));
    std::vector<int32_t> global_tmp;
    if (each) MP_TRY(globalize_roots_arg(ctx, model, n_roots, model_index, root_state, mem_flags, global_tmp, &root_state));
    MP_TRY(wave_roots(ctx, who, root_state, n_roots, model->S, mem));
    // a record per chance node: every step of every episode may expand one decision node
    const long long cap = 1 + ((long long)episodes + 2) * horizon * A;
    MP_TRY(gape_check_capacity(who, cap, sizeof(GapeNode)));
    GapeTables tab;
    MP_TRY(gape_upload_tables(ctx, 42, episodes, horizon, n_actions_env, action_column, host_tab, &tab));

    GapeArgs a;
    a.Sb = model->Sb > 0 ? model->Sb : model->S;
    // (the global form is the launch mp_gape_plan always made: CUs * 32 wavefronts at most, path[H + 1] in LDS)
    const int cus = ctx->prop.multiProcessorCount;
    const EachForm form = each ? each_form(EACH_GAPE, a.Sb, A, horizon, n_roots, cus) : each_form_global(EACH_GAPE, horizon, n_roots, cus);
    a.n_roots = n_roots; a.A = A; a.M = episodes; a.H = horizon; a.cap = (int)cap; a.done_on_next = model->done_on_next;
    a.uniform = continuation; a.n_env = n_actions_env; a.max_plan_len = max_plan_len; a.gamma = gamma; a.accuracy = accuracy;
    a.grid = form.grid; a.rec = model->rec; a.thr = tab.thr; a.vinit = tab.vinit; a.col = tab.col;
    MP_TRY(wave_tree(ctx, 8, n_roots, A, (long)cap, 2, kGapeKeepBytes, a.grid + 1, a.grid, &a.nodes, &a.val, &a.n_nodes_out, &a.keep));
    WaveIo io(mem, rmem, n_roots, root_state, &a.root_state, rng_state, &a.rng);
    gape_results_io(io, {plans, plan_len, episodes_run, status, best_challenger, env_steps, child_count, child_lower, child_upper},
                    &a.out, max_plan_len, A);
    MP_TRY(wave_stage(ctx, io));
    if (each)
        MP_TRY(wave_launch(ctx, form.lds ? gape_kernel<GAPE_EACH_LDS> : gape_kernel<GAPE_EACH_GLOBAL>, a.grid, form.lds_bytes(),
                           gape_each_form_name(form.lds, a.keep), a));
    else
        MP_TRY(wave_launch(ctx, gape_kernel<GAPE_WHOLE>, a.grid, form.lds_bytes(), gape_form_name(a.keep), a));
    return wave_unstage(ctx, io);
}
} // namespace
} // extern "C++"

int mp_gape_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes, int32_t horizon,
                 double gamma, double accuracy, int32_t continuation, int32_t n_actions_env, const int32_t *action_column,
                 const double *thr_by_count, const double *value_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                 int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps, int32_t *status, double *child_lower,
                 double *child_upper, int64_t *child_count, int32_t *best_challenger, int32_t mem)
{
    return gape_plan_impl(ctx, model, n_roots, nullptr, root_state, episodes, horizon, gamma, accuracy, continuation, n_actions_env,
                          action_column, thr_by_count, value_init, rng_state, max_plan_len, plans, plan_len, episodes_run, env_steps,
                          status, child_lower, child_upper, child_count, best_challenger, mem, false);
}

int mp_gape_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                        int32_t episodes, int32_t horizon, double gamma, double accuracy, int32_t continuation,
                        int32_t n_actions_env, const int32_t *action_column, const double *thr_by_count, const double *value_init,
                        uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len, int32_t *episodes_run,
                        int64_t *env_steps, int32_t *status, double *child_lower, double *child_upper, int64_t *child_count,
                        int32_t *best_challenger, int32_t mem)
{
    return gape_plan_impl(ctx, model, n_roots, model_index, root_state, episodes, horizon, gamma, accuracy, continuation,
                          n_actions_env, action_column, thr_by_count, value_init, rng_state, max_plan_len, plans, plan_len,
                          episodes_run, env_steps, status, child_lower, child_upper, child_count, best_challenger, mem, true);
}

const char *mp_gape_form_names(void)
{
    static const std::string names = std::string(gape_form_name(true).s) + "\n" + gape_form_name(false).s;
    return names.c_str();
}

const char *mp_gape_each_form_names(void)
{
    static const std::string names = [] {
        std::string out;
        for (int lds = 1; lds >= 0; --lds)
            for (int keep = 1; keep >= 0; --keep) { out += gape_each_form_name(lds != 0, keep != 0).s; out += '\n'; }
        return out;
    }();
    return names.c_str();
}

int mp_gape_each_form_info(int32_t S_each, int32_t A, int32_t horizon, int32_t n_roots, int32_t cus, int64_t *out)
{
    if (!out) return fail(MP_ERR_ARG, "mp_gape_each_form_info: NULL output");
    if (S_each < 1 || A < 1 || horizon < 1 || n_roots < 1 || cus < 1) return fail(MP_ERR_ARG, "mp_gape_each_form_info: bad arguments");
    const EachForm f = each_form(EACH_GAPE, S_each, A, horizon, n_roots, cus);
    out[0] = (int64_t)f.lds_need; out[1] = f.lds ? 1 : 0; out[2] = f.grid; out[3] = (int64_t)f.lds_bytes();
    out[4] = (int64_t)kEachLdsDefaultBytes; out[5] = (int64_t)kLdsBytes;
    return MP_OK;
}

int mp_gape_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, uint8_t *kind, int32_t *parent, int32_t *action,
                        int32_t *depth, int64_t *count, double *cumulative_reward, double *mu_ucb, double *mu_lcb,
                        double *value_upper, double *value_lower, uint8_t *done, int32_t *state)
{
    int32_t slot, n;
    // (tree kind 8 is what mp_gape_plan and mp_gape_plan_models both leave; after the latter `state` holds GLOBAL states)
    MP_TRY(wave_export_begin(ctx, 8, "mp_gape_tree_export", "mp_gape_plan", root, &slot, &n));
    std::vector<GapeNode> na((size_t)n);
    std::vector<double> val((size_t)n * 2);
    MP_TRY(wave_pull(ctx, WS_TREE0, slot, n, sizeof(GapeNode), na.data()));
    MP_TRY(wave_pull(ctx, WS_TREE1, slot, n, 2 * sizeof(double), val.data()));
    // the records hold a chance node and its decision child: both, in the order they were created
    std::vector<std::pair<int32_t, int32_t>> order; // (creation number, record * 2 + is_chance)
    order.emplace_back(0, 0);
    for (int i = 1; i < n; ++i) {
        if (na[i].cseq < 1 || na[i].parent < 0 || na[i].parent >= n) return fail(MP_ERR_ARG, "mp_gape_tree_export: bad record %d", i);
        order.emplace_back(na[i].cseq, i * 2 + 1);
        if (na[i].dseq >= 0) order.emplace_back(na[i].dseq, i * 2);
    }
    std::sort(order.begin(), order.end());
    const int m = (int)order.size();
    if (n_nodes) *n_nodes = m;
    if (m > cap) return fail(MP_ERR_ARG, "mp_gape_tree_export: capacity %d < %d nodes", cap, m);
    std::vector<int32_t> pos((size_t)n * 2, -1);
    for (int q = 0; q < m; ++q) pos[order[q].second] = q;
    for (int q = 0; q < m; ++q) {
        const int i = order[q].second >> 1;
        const bool chance = order[q].second & 1;
        const GapeNode &r = na[i];
        if (kind) kind[q] = chance ? 1 : 0;
        if (parent) parent[q] = chance ? pos[r.parent * 2] : (i == 0 ? -1 : pos[i * 2 + 1]);
        if (action) action[q] = chance ? r.action : (i == 0 ? -1 : r.state);
        if (depth) depth[q] = chance ? r.depth - 1 : r.depth;
        if (count) count[q] = chance ? r.count_c : r.count_d;
        if (cumulative_reward) cumulative_reward[q] = chance ? 0.0 : r.cum;
        if (mu_ucb) mu_ucb[q] = chance ? 0.0 : r.mu_ucb;
        if (mu_lcb) mu_lcb[q] = chance ? 0.0 : r.mu_lcb;
        if (value_upper) value_upper[q] = chance ? val[2 * (size_t)i] : r.vu;
        if (value_lower) value_lower[q] = chance ? val[2 * (size_t)i + 1] : r.vl;
        if (done) done[q] = chance ? 0 : (uint8_t)r.done;
        if (state) state[q] = chance ? na[r.parent].state : r.state;
    }
    return MP_OK;
}

} // extern "C"
