/*
 * mi355plan.h -- C ABI of libmi355plan.so, the MI355X (gfx950) planning core.
 *
 * The reference (eleurent/rl-agents) is pure Python and has no FFI; this header is the boundary a
 * maintainer binds (ctypes / cffi ABI mode) to replace the bodies of the
 * reference functions cited on each entry point.  Citations are relative to /root/reference.
 *
 * Conventions
 *   - every function returns 0 on success or a negative MP_ERR_* code; it never throws.
 *     mp_last_error() returns a thread-local, human-readable message for the last failure.
 *   - mp_ctx owns one HIP device + one stream + growable device workspaces.  Not thread-safe per
 *     ctx; use one ctx per (process, GPU).
 *   - array arguments are C-contiguous.  `mem` selects where the caller's arrays live:
 *       MP_MEM_HOST   (0): host pointers; the call copies in, runs, copies out and synchronises.
 *       MP_MEM_DEVICE (1): device pointers on the ctx device (e.g. torch tensors' data_ptr());
 *                          the call only enqueues work on the ctx stream and returns.
 *     Output pointers may be NULL when the caller does not want that output.
 *   - all floating point is IEEE double evaluated in the reference's operation order with no
 *     fused multiply-add; integer indices are int32 on the device (tables are accepted as the
 *     int64 numpy arrays the reference holds and range-checked on upload).
 */
#ifndef MI355PLAN_H
#define MI355PLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP_ABI_VERSION 7

#define MP_OK 0
#define MP_ERR_HIP (-1)          /* a HIP runtime call failed (message has the hipError string)  */
#define MP_ERR_REWARD_RANGE (-2) /* OPD: reward outside [0,1] (deterministic.py:46-47 ValueError) */
#define MP_ERR_GAPE_NO_CHALLENGER (-9) /* MDP-GapE status: the root lists one action (mdp_gape.py:247, max() of an empty list: ValueError) */
#define MP_ERR_GAPE_PLACEHOLDERS (-10) /* MDP-GapE status: more next states observed than max_next_states_count (mdp_gape.py:284 ValueError) */
#define MP_ERR_GBOP_PLACEHOLDERS (-11) /* GBOP status: more next states observed than max_next_states_count (graph_based_stochastic.py:217 ValueError) */
#define MP_ERR_GBOP_REWARD_THRESHOLD (-12) /* GBOP status: a reward threshold other than 0 reached the mis-called kl_upper_bound (:79-82 TypeError) */
#define MP_ERR_GBOP_CHOICE_P (-13) /* GBOP status: p_minus fails the checks of Generator.choice in get_plan (:156 ValueError) */
#define MP_ERR_ALLOC (-3)
#define MP_ERR_ARG (-4)          /* invalid argument / unsupported configuration                  */
#define MP_ERR_MODE (-5)         /* model kind not valid for this call ("Unknown mode")           */
#define MP_ERR_OLOP_KEY (-6)     /* OLOP status: the "zeros" continuation's action is not a child (olop.py:89 KeyError) */
#define MP_ERR_GBOPD_DIVERGED (-7)  /* GBOP-D status: a plan made more than 2^22 queue pops (bounds that cycle, never converge) */
#define MP_ERR_GBOPD_NO_ACTION (-8) /* GBOP-D status: a node no action is listed for (graph_based.py:74, np.amax([]) ValueError) */

#define MP_MEM_HOST 0
#define MP_MEM_DEVICE 1
/* OR-ed into MP_MEM_HOST: `rng_state` alone is a DEVICE pointer (an mp_rng, below) while every other array is a host
 * array -- the 48-byte generator record per root then never crosses PCIe (it only has to when Python asks for it). */
#define MP_MEM_RNG_DEVICE 2

/* model kinds (value_iteration.py:51-61 `mode`) */
#define MP_MODE_DETERMINISTIC 0
#define MP_MODE_STOCHASTIC 1
#define MP_MODE_SPARSE 2
#define MP_MODE_CARTPOLE 3

typedef struct mp_ctx mp_ctx;
typedef struct mp_model mp_model;

const char *mp_last_error(void);
int mp_abi_version(void);

/* ---------------------------------------------------------------- context ------------------- */
/* `stream`: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream), or NULL
 * to let the ctx create and own a stream. */
int mp_ctx_create(int device, void *stream, mp_ctx **out);
int mp_ctx_destroy(mp_ctx *ctx);
int mp_ctx_set_stream(mp_ctx *ctx, void *stream);
/* Waits for the ctx's stream.  Returns MP_ERR_ARG -- once, then clears -- when a device-array call since the last
 * synchronisation had to clamp out-of-range roots (mp_uct_plan_models / mp_opd_plan_models with MP_MEM_DEVICE cannot validate
 * model_index / root_state on the host; host arrays are validated before the launch, as the reference's IndexError would be). */
int mp_ctx_synchronize(mp_ctx *ctx);
/* the sticky count behind that (read without clearing; exact only after the work was waited for) */
int mp_ctx_device_faults(mp_ctx *ctx, int32_t *count);
/* the hipStream_t the ctx enqueues on (its own or the caller's): lets the caller order events / collectives after its work */
int mp_ctx_get_stream(mp_ctx *ctx, void **stream);
/* device facts for reports: compute units, wavefront size, LDS bytes per workgroup, HBM bytes */
int mp_ctx_device_info(mp_ctx *ctx, int32_t *n_cu, int32_t *wave_size, int64_t *lds_bytes, int64_t *hbm_bytes,
                       char *name, int32_t name_cap);

/* ---------------------------------------------------------------- host-inclusive fast path --- */
/*
 * SURVEY.md 8(d) measures plan() with host arrays in and out (trainer/evaluation.py:168: agent.plan(observation) is a host
 * call).  Three things make that path fast; none changes a result:
 *   - ZERO-COPY: mp_host_alloc / mp_host_free hand out host memory that is pinned AND mapped into the device's address
 *     space (hipHostMalloc, portable | mapped).  When every array of a MP_MEM_HOST call lies in such memory, the kernels
 *     read the root states from and write the results to the caller's arrays directly over the bus: the call is one
 *     launch and one synchronisation, no copy is issued (every plan entry point; MP_NO_ZERO_COPY=1 disables).
 *     mp_uct_plan does so up to 65 536 roots (MP_ZERO_COPY_MAX); larger batches in such memory run as two chunks on two
 *     streams with asynchronous copies (the first chunk's results travel under the second chunk's kernel: faster than
 *     13 MB of kernel stores over the bus).  Any other host pointer is still accepted everywhere and goes through
 *     staging copies.
 *   - mp_uct_plan with mem = MP_MEM_HOST and ordinary (pageable) arrays splits batches of more than 65 536 roots into
 *     chunks and pipelines H2D(roots) -> kernel -> D2H(results) of different chunks over several HIP streams owned by
 *     the ctx (same kernels, same trees, same results: a root's plan depends on its own state and stream only).
 *     mp_last_kernel_ms then covers the whole pipelined region.  MP_PIPE_CHUNK=<roots> / MP_PIPE_STREAMS=<1..8>
 *     override; MP_PIPE_CHUNK=0 disables.
 *   - mp_rng: generator records resident on the device (see MP_MEM_RNG_DEVICE).
 */
int mp_host_alloc(mp_ctx *ctx, int64_t bytes, void **out);
int mp_host_free(mp_ctx *ctx, void *ptr);
/*
 * n numpy-PCG64 generator records uint64 [n,6] on the device -- the planners' np_random (tree_search/abstract.py:124-131)
 * for a batch of roots, continuing across plan() calls exactly as the host records would.
 *   mp_rng_set / mp_rng_get copy records [first, first+count) from / to a host array (synchronous).
 *   mp_rng_seed_sequence fills them as Generator(PCG64(SeedSequence(entropy + [first_key + i]))) for record first + i:
 *   `entropy` = n_words uint32 words (numpy's little-endian split of the entropy integers), the root's global index is
 *   appended as one more entropy integer -- rl_agents_amd's batch streams (AbstractPlanner.batch_rng_states).  Computed
 *   on the host in C (numpy's SeedSequence hashing restated; tests compare with numpy) and uploaded.
 *   mp_rng_device_ptr: the device address of record `first`, to pass as `rng_state` with MP_MEM_RNG_DEVICE (or with
 *   MP_MEM_DEVICE).
 * mp_seed_sequence_states is the host-only half: out uint64 [count,6].
 */
typedef struct mp_rng mp_rng;
int mp_rng_create(mp_ctx *ctx, int32_t n, mp_rng **out);
int mp_rng_free(mp_rng *rng);
int mp_rng_set(mp_rng *rng, int32_t first, int32_t count, const uint64_t *state6);
int mp_rng_get(mp_rng *rng, int32_t first, int32_t count, uint64_t *state6);
int mp_rng_seed_sequence(mp_rng *rng, int32_t first, int32_t count, const uint32_t *entropy, int32_t n_words,
                         int64_t first_key);
uint64_t *mp_rng_device_ptr(mp_rng *rng, int32_t first);
int mp_seed_sequence_states(const uint32_t *entropy, int32_t n_words, int64_t first_key, int32_t count, uint64_t *out);

/* ---------------------------------------------------------------- transition models ---------- */
/*
 * Deterministic finite-MDP tables: what the planners reach through env.step on a FiniteMDPEnv
 * (tree_search/abstract.py:158-161) and value iteration through mdp.transition / mdp.reward /
 * mdp.terminal (dynamic_programming/value_iteration.py:52-53,62-63).  Replaces
 * common/factory.py:119-134 safe_deepcopy_env: a cloned environment is an (int32 state,
 * int32 steps) pair on the device.
 *   transition int64 [M,S,A], reward double [M,S,A], terminal uint8 [S] or NULL.
 *   M > 1 = several models of one MDP (robust_value_iteration.py:21-27); tree search uses model 0.
 *   done_on_next: 0 -> terminated = terminal[s] (state acted FROM), 1 -> terminal[s'].
 *   max_steps: TimeLimit-style truncation for rollouts, 0 = none.
 * Always host pointers (model upload is outside every timed region).
 */
int mp_model_load_table(mp_ctx *ctx, int32_t M, int32_t S, int32_t A, const int64_t *transition,
                        const double *reward, const uint8_t *terminal, int32_t done_on_next, int32_t max_steps,
                        mp_model **out);
/*
 * A BATCH of N independent deterministic finite MDPs of one shape (S states, A actions each), one per episode of a
 * benchmark batch.  The reference evaluates one environment per process (trainer/evaluation.py:139-194,
 * scripts/experiments.py:102-106) and, for an environment that is not a FiniteMDPEnv (highway-v0), re-extracts its own
 * table with to_finite_mdp() at EVERY step (dynamic_programming/value_iteration.py:29-35, tree_search/abstract.py:59-62
 * through env_preprocessors): a batch of such episodes is N distinct tables, all of which change between two steps.
 *   transition int64 [N,S,A] (state indices LOCAL to each MDP, 0 <= t < S), reward double [N,S,A],
 *   terminal uint8 [N,S] or NULL; done_on_next / max_steps as mp_model_load_table.  N * S * A < 2^31.
 * The result is ONE table model over the disjoint union of the N state spaces -- GLOBAL state b * S + s, records packed
 * exactly as mp_model_load_table packs them -- so that every entry point that takes a deterministic table model works
 * on it unchanged and a root's plan depends on its own MDP only: mp_uct_plan*, mp_opd_plan, mp_ropd_plan,
 * mp_saopd_*, mp_policy_load* (per-state policies over the N * S global states), mp_env_step, mp_greedy_actions take
 * GLOBAL states; mp_uct_plan_models / mp_opd_plan_models below take (model_index, local state) pairs instead.
 * Tree exports report global states.  mp_vi_solve on it would test convergence over all N MDPs at once, which is not what
 * N agents do: use mp_vi_solve_batch (mp_vi_solve refuses a batch model).
 * mp_model_batch_info: *N = number of MDPs (1 for any other model), *S_each = states per MDP.
 */
int mp_model_load_table_batch(mp_ctx *ctx, int32_t N, int32_t S, int32_t A, const int64_t *transition, const double *reward,
                              const uint8_t *terminal, int32_t done_on_next, int32_t max_steps, mp_model **out);
int mp_model_batch_info(const mp_model *model, int32_t *N, int32_t *S_each);
/*
 * Replace the tables of MDPs [first, first + count) of a batch model (or, with first = 0 and count = 1, the whole of a
 * single-MDP table model from mp_model_load_table with M = 1): the per-step delta of a batch of highway episodes is each
 * episode's own table.  Arrays as mp_model_load_table_batch with N = count (host pointers; terminal must be given iff the
 * model was loaded with terminal flags).  Stream-ordered on the ctx stream through a pinned staging block owned by the
 * model: work enqueued earlier still reads the old tables, work enqueued later the new ones; nothing is synchronised
 * unless the previous update's copies are still in flight.  Only the touched records are re-packed.  Policies loaded for
 * the model become invalid (their fused records hold the old transitions).
 */
int mp_model_update_tables(mp_model *model, int32_t first, int32_t count, const int64_t *transition, const double *reward,
                           const uint8_t *terminal);
/*
 * Delta upload of a changed model (value_iteration.py:12-21,29-35 re-converts the env on every act):
 * replace n_rows rows of a deterministic table model (single, M = 1, or batch).
 *   rows int32 [n_rows]: GLOBAL state ids, distinct;  transition int64 [n_rows,A] (LOCAL next-state indices of the row's
 *   MDP), reward double [n_rows,A], terminal uint8 [n_rows] or NULL = the rows' terminal flags do not change.
 * With terminal == NULL only the records of the listed rows are re-packed; otherwise every record of the MDPs that own a
 * listed row is (a record carries terminal[next]: predecessors of a row whose flag changed must follow).  Stream-ordered
 * like mp_model_update_tables.
 */
int mp_model_update_rows(mp_model *model, int32_t n_rows, const int32_t *rows, const int64_t *transition, const double *reward,
                         const uint8_t *terminal);
/*
 * Environments that restrict the actions available in a state -- state.get_available_actions(), read by
 * DeterministicNode.expand (deterministic.py:32-35) -- as a table:
 *   available uint8 [S,A], non-zero = action a is listed in state s; every state needs at least one (else MP_ERR_ARG).
 * Host pointer.  Applies to the deterministic table model it is called on; mp_opd_plan then expands the available
 * actions only.  Policies loaded earlier for the model become invalid.  (MCTS reads availability through its POLICIES,
 * mcts.py:59-97: see mp_policy_load_listed.)  A whole dense or sparse model takes the table too and only keeps it: Sparse
 * Sampling reads it (sparse_sampling.py:40-43); the stochastic UCT entry points go on refusing a restricted model without a policy.
 */
int mp_model_set_available(mp_model *model, const uint8_t *available);
/*
 * Dense stochastic model (value_iteration.py:54-55, robust_value_iteration.py:55-56):
 *   transition double [M,S,A,S], reward double [M,S,A], terminal uint8 [S] or NULL.
 * mem = MP_MEM_DEVICE borrows the caller's device arrays (no copy; they must outlive the model).
 */
int mp_model_load_dense(mp_ctx *ctx, int32_t M, int32_t S, int32_t A, const double *transition,
                        const double *reward, const uint8_t *terminal, int32_t mem, mp_model **out);
/*
 * A block of source-state rows of a dense model, for value iteration sharded over GPUs: this
 * rank owns rows [row0, row0 + S_rows) of every model, i.e. transition double [M,S_rows,A,S_cols] (S_cols = |S|),
 * reward double [M,S_rows,A], terminal uint8 [S_rows] (flags of the owned rows) or NULL.  Use with mp_vi_backup.
 */
int mp_model_load_dense_rows(mp_ctx *ctx, int32_t M, int32_t S_rows, int32_t A, int32_t S_cols,
                             const double *transition, const double *reward, const uint8_t *terminal, int32_t mem,
                             mp_model **out);
/* Sparse model (value_iteration.py:56-59): transition double [S,A,B], next int64 [S,A,B]. */
int mp_model_load_sparse(mp_ctx *ctx, int32_t S, int32_t A, int32_t B, const double *transition,
                         const int64_t *next, const double *reward, const uint8_t *terminal, mp_model **out);
/*
 * Closed-form CartPole (gymnasium CartPole-v0/v1 dynamics, absent from this image; restated in
 * rl_agents_amd/envs/cartpole.py).  A clone is (x, x_dot, theta, theta_dot, steps).
 */
typedef struct {
    double gravity, masscart, masspole, length, force_mag, tau;
    double theta_threshold, x_threshold;
    int32_t max_steps;       /* TimeLimit: 200 for CartPole-v0 */
    int32_t euler;           /* 1 = explicit Euler (gymnasium default) */
} mp_cartpole_params;
int mp_model_load_cartpole(mp_ctx *ctx, const mp_cartpole_params *params, mp_model **out);
/*
 * CartPole's dynamics take math.sin / math.cos of the pole angle (gymnasium's cartpole.py, restated in
 * rl_agents_amd/envs/cartpole.py), i.e. the host C library's sin / cos -- which are not correctly rounded: "the" value is
 * what glibc's algorithm yields.  The kernels evaluate glibc's dbl-64 algorithm for |x| < 0.855469 themselves (a pole angle
 * stays below 0.21 rad), in the form that reproduces THIS host's libm:
 *   mp_libm_sincos_variant(): 1 = the FMA-contracted form (x86-64 CPUs with FMA + AVX2), 2 = every operation rounded
 *   (SSE2 / AVX variants), 0 = neither matched the host's sin / cos on the probe sample -- the device then uses its own
 *   math library and CartPole plans carry the tolerance of rounds 1-4 (>= 99.5 % of roots identical); host only, cached.
 *   mp_libm_sincos: the restated functions on the HOST, variant 1 / 2 (0 = libm itself): s[i], c[i] = sin, cos of x[i].
 *   mp_selftest_sincos: the same on the DEVICE (host arrays in / out) -- tests compare 10^7 angles with the host's libm;
 *   variant 3 / 4: the branch-free forms of variant 1 / 2 that the CartPole rollouts evaluate (|x| < 0.855 only).
 */
int mp_libm_sincos_variant(void);
int mp_libm_sincos(int32_t n, const double *x, int32_t variant, double *s, double *c);
int mp_selftest_sincos(mp_ctx *ctx, int32_t n, const double *x, int32_t variant, double *s, double *c);
int mp_model_free(mp_model *model);
int mp_model_info(const mp_model *model, int32_t *mode, int32_t *M, int32_t *S, int32_t *A, int32_t *B);

/* ---------------------------------------------------------------- value iteration ----------- */
/*
 * ValueIterationAgent.get_state_action_value (value_iteration.py:42-45) =
 * fixed_point_iteration (:65-73) of bellman_expectation(best_action_value(q)) (:47-63) from
 * Q0 = 0, with numpy.allclose(rtol, atol) early exit returning the PREVIOUS iterate; and, with
 * robust = 1, RobustValueIterationAgent.get_state_action_value (robust_value_iteration.py:39-58):
 * min over the M models, no terminal masking.
 *   Q_out double [S,A]; sweeps_out int32 [1] = Bellman sweeps actually executed.
 * Deterministic and sparse modes are bit-exact with the reference.  The dense mode has two forms (mp_vi_dense_mode):
 * in numpy's own order of roundings and additions -- bit-exact Q, V and sweep counts (the default) -- or on the f64
 * matrix cores, which accumulate in another order than numpy's pairwise sum (relative error ~1e-15 per sweep: Q within
 * 1e-12, greedy actions equal, sweep count within 1).
 * Deterministic models with |S| <= 16 384 are solved by ONE persistent launch whose workgroups hand V to each other and
 * therefore must all be resident at once.  On a GPU shared with other work that can fail (bounded spins, no hang):
 *   mem = MP_MEM_HOST  : the call notices and transparently solves again on the chained launches;
 *   mem = MP_MEM_DEVICE: asynchronous, nothing is read back: sweeps_out[0] = -1 and NaN in Q_out report the failure --
 *                        check sweeps_out, or set MP_VI_NO_PERSIST=1 to always use the chained launches.
 */
int mp_vi_solve(mp_ctx *ctx, mp_model *model, double gamma, int32_t iterations, double rtol, double atol,
                int32_t robust, double *Q_out, int32_t *sweeps_out, int32_t mem);
/*
 * N value-iteration agents at once: mp_vi_solve of every MDP of a batch model (mp_model_load_table_batch) in ONE launch,
 * one workgroup per MDP -- the fixed-point iteration of each MDP runs to ITS OWN allclose exit, exactly as N
 * ValueIterationAgent objects would (value_iteration.py:42-45,65-73 per agent; trainer/evaluation.py:139-194 runs one
 * agent per process).  Bit-exact with N mp_vi_solve calls on the N tables.
 *   Q_out double [N,S,A] (= [N*S, A] over global states: what mp_greedy_actions takes), sweeps_out int32 [N];
 *   either may be NULL (that output is not written).
 * mem = MP_MEM_DEVICE only enqueues.  Rows of an MDP live in registers and its value vector in LDS when
 * S <= 4096 (any such S), else the value vector is double-buffered in LDS (S <= 10 200) or kept in global memory.
 * Batches of few large MDPs run K = 2 / 4 / 8 workgroups per MDP that must all be resident at once; on a GPU shared with
 * other work a cluster that does not meet gives up (bounded spins, no hang) and the MDP is solved again by a follow-up
 * launch of the same call -- in both memory modes the caller receives the exact result, never a failure report.
 */
int mp_vi_solve_batch(mp_ctx *ctx, mp_model *model, double gamma, int32_t iterations, double rtol, double atol,
                      double *Q_out, int32_t *sweeps_out, int32_t mem);
/* get_state_value (value_iteration.py:37-40): the V-form iteration.  V_out double [S]. */
int mp_vi_solve_v(mp_ctx *ctx, mp_model *model, double gamma, int32_t iterations, double rtol, double atol,
                  double *V_out, int32_t mem);
/* RobustValueIterationAgent.get_state_value (robust_value_iteration.py:32-37): V <- max_a min_m (R_m + gamma next_v_m(V)),
 * allclose on V, no terminal masking; deterministic and dense models. */
int mp_vi_solve_v_robust(mp_ctx *ctx, mp_model *model, double gamma, int32_t iterations, double rtol, double atol,
                         double *V_out, int32_t mem);
/*
 * One Bellman backup of a dense (or row-block) model: Q[rows,A] = min_m (R_m + gamma * mask(T_m . V)), the body of
 * bellman_expectation (value_iteration.py:54-55,62-63; robust_value_iteration.py:46-58).  V double [S_cols] in,
 * Q double [S_rows,A] out.  The row-sharded driver (rl_agents_amd/distributed.py) all_gathers V between backups.
 */
int mp_vi_backup(mp_ctx *ctx, mp_model *model, double gamma, int32_t robust, const double *V, double *Q, int32_t mem);
/*
 * How dense models (MP_MODE_STOCHASTIC) are contracted with V by every VI entry point of this ctx
 * (value_iteration.py:54-55: (T * v).sum(axis=-1) -- products rounded one by one, numpy's pairwise add.reduce):
 *   MP_VI_DENSE_MFMA   v_mfma_f64_16x16x4_f64 (fused, reordered accumulation): tolerance parity, see mp_vi_solve
 *   MP_VI_DENSE_EXACT  the reference's order restated (eight strided accumulators per block of <= 128 elements, the
 *                      halving recursion above it): bit-exact; both stream T once and are bound by HBM
 * Without a call the environment decides (MP_VI_DENSE=mfma|exact), else MP_VI_DENSE_EXACT: parity first, and at
 * 0.25 flop per byte the contraction is bound by HBM in both forms (measured: DESIGN.md 4.5).
 */
#define MP_VI_DENSE_MFMA 0
#define MP_VI_DENSE_EXACT 1
int mp_vi_dense_mode(mp_ctx *ctx, int32_t mode);
/* Host only (no GPU needed): the tables MP_VI_DENSE_EXACT sums a row of n elements by -- numpy's add.reduce: the
 * running sum, from the identity 0., of the pairwise sums (DOUBLE_pairwise_sum: blocks of at most 128, halves rounded
 * down to a multiple of 8) of the row's pieces of numpy.getbufsize() = 8192 elements.
 * leaves int32 [cap_leaves,2] {offset, length} left to right, leaf 0 = {0, 0} is the identity; nodes int32 [cap_nodes,2] {left, right} result
 * slots of the recursion's additions ordered by height (leaf l = slot l, addition k = slot n_leaves + k, the last one
 * is the row's sum); hoff int32 [cap_heights + 1]: additions of height h + 1 are [hoff[h], hoff[h+1]);
 * counts int32 [4] = {n_leaves, n_nodes, n_heights, most 8-element steps in a leaf}.  Arrays too small (or NULL) are
 * left alone: call once for the counts.  tests/test_host_logic.py replays the tables against numpy.add.reduce. */
int mp_vi_exact_plan(int32_t n, int32_t cap_leaves, int32_t *leaves, int32_t cap_nodes, int32_t *nodes, int32_t cap_heights,
                     int32_t *hoff, int32_t *counts);
/* Timing hook: run exactly `sweeps` Bellman sweeps (no early exit), Q left on the device. */
int mp_vi_sweeps(mp_ctx *ctx, mp_model *model, double gamma, int32_t sweeps, int32_t robust);
/* The names the single-model entry points above (solve, solve_v, solve_v_robust, sweeps, backup) record for
 * mp_last_kernel_variant, one per line (host only; they are not part of mp_kernel_form_names): the form of the launch that
 * produced the returned values -- after the persistent kernel's host-mode fallback the chained one.
 *   vi_det_small_a{2,3,4,5,6,8,any}             deterministic tables, one workgroup, everything in LDS
 *   vi_det_persist_a{A}_m{M}                    ... one persistent grid (19 pairs of |A| and models)
 *   vi_det_chain_a{2,3,4,5,6,8,any}[_graph]     ... a launch per sweep; _graph: replayed from the captured graph
 *   vi_sparse, vi_sparse_big                    sparse models with up to / more than 128 next states
 *   vi_dense_exact_n{8,10,12,14,16}_{lds,pieces,global}   dense rows in numpy's order: unrolled steps of a leaf, where V is read from
 *   vi_dense_mfma, vi_dense_mfma_split          dense rows on the matrix cores, the columns in one / several segments
 * A solve of 0 iterations on the chained, dense or sparse path launches no sweep and records the empty name. */
const char *mp_vi_form_names(void);
/* How many times this context has captured a chain of deterministic sweeps into a graph (vi_det_chain_*_graph).  The context
 * keeps the executable graph of its last chain, keyed by everything baked into the kernel arguments (model, table and
 * workspace pointers, sizes, iterations, gamma, tolerances, Q or V form): a call with that key replays it and leaves the
 * count alone, any other captures anew.  The tables are read through their pointers, so a replay after an in-place
 * mp_model_update_tables solves the new tables.  Host only; 0 for a NULL context. */
int64_t mp_vi_graph_captures(mp_ctx *ctx);
/* Host arithmetic of those launches (no device; the launch code calls the same functions), on a device of `cus` compute units.
 * The MP_VI_* and MP_DENSE_NO_SPLIT knobs are read from the environment.  out int64 [14]:
 *   mode = MP_MODE_DETERMINISTIC, M models of S states and A actions (Sc ignored):
 *     [0] LDS bytes of the single-workgroup kernel's tables, [1] 1 if they fit, [2] 1 if that kernel is taken (MP_VI_NO_SMALL),
 *     [3] threads per workgroup and [4] workgroups of the persistent grid, [5] 1 if the persistent kernel is admitted
 *     (it is taken when [2] is 0);
 *   mode = MP_MODE_STOCHASTIC, rows of Sc columns (S, A, M ignored):
 *     [6] most 8-element steps in a leaf (nb) and [7] the unrolled form NBT it selects, [8] waves per workgroup, [9] LDS bytes
 *     of the summation tables, [10] where V goes by default and [11] with the knobs: 0 read through L2, 1 all of it in LDS,
 *     2 in pieces of 8192; [12] column segments of the matrix-core form, [13] columns per segment.
 * The other half of `out` is zero. */
int mp_vi_geometry(int32_t mode, int32_t S, int32_t A, int32_t M, int32_t Sc, int32_t cus, int64_t *out);
/* The kernel form mp_vi_solve_batch chooses for N MDPs of Sb states and A actions on a device of `cus` compute units (host only;
 * the solve launches from the same function).  The MP_VI_BATCH_* knobs are read from the environment as the solve reads them.
 *   out int64 [7]: [0] form (0 register, 1 cluster, 2 streaming workgroup, 3 LDS workgroup, 4 global-memory workgroup),
 *                  [1] the compile-time |A| (0: the loop form), [2] states a thread keeps in registers (0: none), [3] threads per
 *                  workgroup, [4] workgroups per MDP, [5] workgroups of the launch, [6] dynamic LDS bytes.
 *   *name:         the form, as mp_last_kernel_variant names it (static storage).
 * MP_ERR_ARG for a NULL argument or a size below 1; iterations may be 0. */
int mp_vi_batch_geometry(int32_t N, int32_t Sb, int32_t A, int32_t iterations, int32_t cus, int64_t *out, const char **name);

/* ---------------------------------------------------------------- UCT ----------------------- */
/*
 * MCTS.plan (tree_search/mcts.py:179-184) for n_roots independent roots: `episodes` iterations of
 * MCTS.run (:132-158: select by MCTSNode.selection_strategy :275-286 with random tie-break
 * abstract.py:296-311, expand :237-246, rollout MCTS.evaluate :160-177, backup
 * MCTSNode.update_branch :248-265), then AbstractPlanner.get_plan (abstract.py:143-156) with
 * MCTSNode.selection_rule (mcts.py:212-218).  Open loop (closed_loop = False).
 *   root_state  : table model int32 [n_roots]; cartpole double [n_roots,4]
 *   root_steps  : int32 [n_roots] env.steps at plan time (TimeLimit), or NULL = 0
 *   prior_p     : double [A]  prior over actions 0..A-1   (mcts.py:46-97 policies)
 *   rollout_p   : double [A]  rollout distribution; sampled as numpy Generator.choice(p=...)
 *   rng_state   : uint64 [n_roots,6] numpy PCG64 state {state_hi, state_lo, inc_hi, inc_lo,
 *                 has_uint32, uinteger}; advanced in place exactly as the reference's
 *                 planner.np_random would be (so plans are bit-identical at equal seeds)
 *   plans       : int32 [n_roots,max_plan_len], -1 padded;  plan_len int32 [n_roots]
 *   root_value  : double [n_roots];  root_child_count int64 [n_roots,A];
 *   root_child_value double [n_roots,A];  env_steps int64 [n_roots] (= len(planner.observations))
 */
int mp_uct_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const void *root_state, const int32_t *root_steps,
                int32_t episodes, int32_t horizon, double gamma, double temperature, const double *prior_p,
                const double *rollout_p, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                int32_t *plan_len, double *root_value, int64_t *root_child_count, double *root_child_value,
                int64_t *env_steps, int32_t mem);
/*
 * mp_uct_plan on a batch model (mp_model_load_table_batch) with one MDP per root: root i plans on MDP model_index[i]
 * from its LOCAL state root_state[i] (model_index int32 [n_roots], values in [0, N); several roots may share an MDP).
 * Everything else as mp_uct_plan; equal to mp_uct_plan with root_state = model_index * S + root_state.
 */
int mp_uct_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                       const int32_t *root_steps, int32_t episodes, int32_t horizon, double gamma, double temperature,
                       const double *prior_p, const double *rollout_p, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                       int32_t *plan_len, double *root_value, int64_t *root_child_count, double *root_child_value,
                       int64_t *env_steps, int32_t mem);
/*
 * Per-state prior / rollout policies: MCTSWithPriorPolicyAgent (tree_search/mcts_with_prior.py:8-71) replaces the
 * planner's two policies by agent_policy_available (:47-62), the action distribution a prior agent gives for the state
 * the policy is asked about.  On a finite MDP that is a table:
 *   prior   double [S,A]  prior[s,a]   = probability handed to MCTSNode.expand when a node reached in state s is expanded
 *   rollout double [S,A]  rollout[s,:] = distribution MCTS.evaluate samples from in state s (Generator.choice(p=...))
 * Host pointers (policy upload is outside every timed region, like model upload).  Any |A| >= 2: mp_uct_plan_policy
 * (nodes' policy rows in registers) plans with 2..8 actions; beyond that mp_uct_plan_stochastic_policy does -- its loop
 * forms take any number of actions and deterministic tables as well as stochastic / sparse models.
 * A policy is tied to the model it was loaded for (its records are fused into the policy tables): use it with that
 * model only (checked) and free it before the model.
 * mp_uct_plan_policy = mp_uct_plan with (prior_p, rollout_p) looked up per state; everything else is identical,
 * including mp_uct_step_tree / mp_uct_tree_export on the trees it leaves.
 */
typedef struct mp_policy mp_policy;
int mp_policy_load(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout, mp_policy **out);
/*
 * Policies over restricted action sets: random_available_policy / preference_policy (mcts.py:59-97) and
 * agent_policy_available (mcts_with_prior.py:56-62) list, for a state, only the actions state.get_available_actions()
 * returns; MCTSNode.expand (mcts.py:237-246) creates one child per LISTED action and the exploration term scales with
 * len(children) = their number (mcts.py:286).
 *   listed uint8 [S,A]: non-zero = the prior policy lists action a in state s (an action may be listed with prior
 *   probability 0: it still gets a child); NULL = every action in every state (= mp_policy_load).  At least one action
 *   per state.  Unlisted actions must have rollout probability 0 unless the rollout policy ignores availability
 *   (random_policy, mcts.py:46-57) -- rollout[s,:] is simply the distribution to sample from.  |A| <= 8.
 */
int mp_policy_load_listed(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout,
                          const uint8_t *listed, mp_policy **out);
/* mp_policy_load_listed + the order in which the ROLLOUT policy lists the actions of each state: rollout_slot uint8 [S, A],
 * slot k of state s is column rollout_slot[s, k] (a permutation per state, zero-probability columns last; NULL = the
 * column order).  The columns -- the order of a node's children and of every tie-break -- follow the PRIOR policy's
 * listing; the rollout's inverse CDF (mcts.py:172, np_random.choice(actions, p=...)) runs over ITS listing.  The two
 * differ when one of them is the `random` policy, which lists np.arange(n) whatever the environment lists (mcts.py:46-57),
 * on an environment whose get_available_actions() is not ascending (highway-env: IDLE first). */
int mp_policy_load_ordered(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout,
                           const uint8_t *listed, const uint8_t *rollout_slot, mp_policy **out);
/* mp_policy_load_ordered with `rows` distribution rows: rows = S (one per state of the model), or rows = the states of ONE MDP
 * of a batch model (mp_model_load_table_batch) -- prior / rollout / listed / rollout_slot are then [rows, A] over LOCAL states
 * and serve every MDP of the batch: the planner's own policies (mcts.py:46-97) on a batch of environments that restrict their
 * actions identically (trainer/evaluation.py:139-194 run N at a time).  Deterministic table models with 2..8 actions and at
 * least 16 384 (s, a) pairs -- and every tiled call -- are fused by kernels on the device (ABI 7); results are identical. */
int mp_policy_load_rows(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout,
                        const uint8_t *listed, const uint8_t *rollout_slot, int32_t rows, mp_policy **out);
int mp_policy_free(mp_policy *policy);
int mp_uct_plan_policy(mp_ctx *ctx, mp_model *model, mp_policy *policy, int32_t n_roots, const void *root_state,
                       const int32_t *root_steps, int32_t episodes, int32_t horizon, double gamma, double temperature,
                       uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len, double *root_value,
                       int64_t *root_child_count, double *root_child_value, int64_t *env_steps, int32_t mem);
/*
 * AbstractPlanner.step_tree with step_strategy "subtree" (abstract.py:172-206): before the next mp_uct_plan, replace
 * the tree of every root left on this ctx by the last mp_uct_plan with the subtree of the root's child `actions[i]`
 * (a root that was never expanded starts a fresh tree, like step_by_reset).  The next mp_uct_plan must have the same
 * n_roots and model; it then continues on the kept statistics instead of starting from empty roots.
 * mp_uct_reset_tree drops the kept trees (step_by_reset, mcts.py:129-130).
 */
int mp_uct_step_tree(mp_ctx *ctx, int32_t n_roots, const int32_t *actions, int32_t mem);
/*
 * The same step for a batch that changes: episodes of a lock-step evaluation end at different steps, and only the live ones
 * plan on (abstract.py:172-206 once per live agent).  The next plan has n_new roots; new root j continues the subtree under
 * child actions[j] of OLD root source_root[j] -- the old roots in any order, one of them for several new roots if wanted;
 * old roots that are not named are dropped.  Serves every tree mp_uct_step_tree serves (mp_uct_plan / _policy / _models and
 * the open-loop trees of mp_uct_plan_stochastic / _policy, stored priors included), with its rules: a root that was never
 * expanded, or an action that is not a child (the slot of an unlisted action), starts a fresh tree; a step that arrives
 * before the plan of the previous one descends one more level, its sources counting the previous step's roots.
 * Host arrays: MP_ERR_ARG, with the trees untouched, for n_new < 1, a source outside [0, n_old) or a ctx without such trees
 * (closed-loop trees among them).  MP_MEM_DEVICE (only enqueues): a source outside the old batch starts a fresh tree.
 * Until the next plan the tree exports refuse (the buffers hold the old batch); mp_uct_reset_tree drops the selection.
 */
int mp_uct_step_tree_select(mp_ctx *ctx, int32_t n_new, const int32_t *source_root, const int32_t *actions, int32_t mem);
int mp_uct_reset_tree(mp_ctx *ctx);
/* Node capacity per root of the trees currently on this ctx (array size for mp_uct_tree_export). */
int mp_uct_tree_capacity(mp_ctx *ctx, int32_t *cap);
/* Tree of root `root` after the last mp_uct_plan on this ctx, creation order (root = node 0, the
 * children of an expanded node are contiguous: first_child, n_children of them -- |A|, or the number of actions a
 * listed policy lists in the node's state).  Host arrays of capacity `cap` nodes. */
int mp_uct_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *action,
                       int64_t *count, double *value, int32_t *first_child, int32_t *n_children);
/* Visit count of the node reached from root `root` by the action sequence `actions[0..n)` (host array) in the trees of the
 * last mp_uct_plan on this ctx -- what `AbstractPlanner.get_plan` (abstract.py:143-156) needs to know about the LAST
 * node of a closed-loop plan (an unvisited action node has no observation child yet) without exporting the tree.
 * *count = -1 when the path leaves the tree (a node on it is not expanded, or the action is not listed there). */
int mp_uct_path_count(mp_ctx *ctx, int32_t root, const int32_t *actions, int32_t n, int64_t *count);

/*
 * MCTS on STOCHASTIC finite MDPs (the `stochastic` [S,A,S] and `sparse` [S,A,B] modes of a finite-MDP env: models from
 * mp_model_load_dense / mp_model_load_sparse; deterministic table models are accepted too), open or closed loop.
 * The reference's planner steps deep copies of the env (mcts.py:183, tree_search/abstract.py:158-161) and the env
 * samples its next state with its OWN numpy generator, next = rng.choice(n, p=transition[s, a]); a copy carries a copy
 * of that generator (common/factory.py:119-134), so every episode of a plan starts from the same env generator state:
 *   env_rng_state uint64 [n_roots,6]: the env generator's record at plan time, read-only (NULL for deterministic models).
 * closed_loop != 0 (mcts.py:147, MCTSNode.get_child :267-273): an action node has one child per distinct observation
 * (= next state index) seen after it, created on first visit; `plans` then alternates action, observation key, action ...
 * as AbstractPlanner.get_plan walks such a tree (abstract.py:143-156); max_plan_len counts both.
 * prior_p / rollout_p: one distribution over the |A| actions for every state (restricted action sets and per-state
 * policies: mp_uct_plan_stochastic_policy below).  mp_model_set_episode_rules sets what a
 * table model gets at load time: done_on_next (terminated = terminal[s'] instead of terminal[s]) and the TimeLimit.
 * mp_uct_stoch_tree_export: the tree of `root` in creation order -- parent, key (action id or observed state), is_obs,
 * count, value -- a node's children in dict order are its children by ascending index; capacity from
 * mp_uct_stoch_tree_capacity.
 */
int mp_model_set_episode_rules(mp_model *model, int32_t done_on_next, int32_t max_steps);
int mp_uct_plan_stochastic(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, const int32_t *root_steps,
                           int32_t episodes, int32_t horizon, double gamma, double temperature, const double *prior_p,
                           const double *rollout_p, int32_t closed_loop, uint64_t *rng_state, const uint64_t *env_rng_state,
                           int32_t max_plan_len, int32_t *plans, int32_t *plan_len, double *root_value,
                           int64_t *root_child_count, double *root_child_value, int64_t *env_steps, int32_t mem);
/* The same plan with PER-STATE policies (restricted action sets, mcts.py:59-97; prior agents, mcts_with_prior.py:47-62) from
 * mp_policy_load / _listed / _ordered on this model -- stochastic, sparse, or a deterministic table (whose per-state policies
 * over more than 8 actions plan here: the loop forms take any number of actions).  A node is expanded with the listed actions and
 * priors of the state the env clone is in at that moment (mcts.py:151-154,237-246) and keeps them -- in open loop later
 * episodes reach it in other states.  mp_uct_step_tree re-uses open-loop trees of either form. */
/*
 * AbstractPlanner.get_visits (abstract.py:163-167): the planner appends the observation of EVERY env step of a plan --
 * descent and rollouts -- to planner.observations (:158-161) and get_visits counts them.  Arms the NEXT
 * mp_uct_plan_stochastic / _policy call of this ctx (host arrays): visits int32 [n_roots, S] receives, per root, how often
 * the plan's env steps landed in each state (= observation of a finite MDP).  Rollouts leave no trace in the tree, so a
 * binding that wants get_visits replays the plan with its saved generator records through this pair
 * (rl_agents_amd/agents/tree_search/mcts.py: a private ctx, so the trees of the real plans stay untouched).
 */
int mp_uct_record_visits(mp_ctx *ctx, int32_t *visits);
int mp_uct_plan_stochastic_policy(mp_ctx *ctx, mp_model *model, mp_policy *policy, int32_t n_roots, const int32_t *root_state,
                                  const int32_t *root_steps, int32_t episodes, int32_t horizon, double gamma, double temperature,
                                  int32_t closed_loop, uint64_t *rng_state, const uint64_t *env_rng_state, int32_t max_plan_len,
                                  int32_t *plans, int32_t *plan_len, double *root_value, int64_t *root_child_count,
                                  double *root_child_value, int64_t *env_steps, int32_t mem);
/* stored child priors (0 for the root and observation nodes) of the tree LAST exported by mp_uct_stoch_tree_export, same order */
int mp_uct_stoch_tree_priors(mp_ctx *ctx, int32_t cap, double *prior);
int mp_uct_stoch_tree_capacity(mp_ctx *ctx, int32_t *cap);
int mp_uct_stoch_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *key,
                             uint8_t *is_obs, int64_t *count, double *value);

/* ---------------------------------------------------------------- OPD ----------------------- */
/*
 * OptimisticDeterministicPlanner.plan (tree_search/deterministic.py:116-122) for n_roots
 * independent roots: budget // A times run() (:106-114: leaf = first maximal upper bound in
 * leaves order :110, DeterministicNode.expand :28-43 with update :45-65, backup_to_root :74-79),
 * then get_plan (abstract.py:143-156) with DeterministicNode.selection_rule (:21-26, random
 * tie-break on exactly equal lower bounds through rng_state).
 *   status int32 [n_roots]: MP_OK or MP_ERR_REWARD_RANGE per root (the reference raises).
 */
int mp_opd_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t budget,
                double gamma, double terminal_reward, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                int32_t *plan_len, double *root_lower, double *root_upper, int64_t *env_steps, int32_t *status,
                int32_t mem);
/* mp_opd_plan on a batch model with one MDP per root (see mp_uct_plan_models): model_index int32 [n_roots], root_state LOCAL. */
int mp_opd_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                       int32_t budget, double gamma, double terminal_reward, uint64_t *rng_state, int32_t max_plan_len,
                       int32_t *plans, int32_t *plan_len, double *root_lower, double *root_upper, int64_t *env_steps,
                       int32_t *status, int32_t mem);
/* Tree of root `root` after the last mp_opd_plan, creation order (the n_children children of an expanded node are
 * contiguous from first_child: |A|, or the available actions of its state); host arrays, capacity `cap`. */
int mp_opd_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *action,
                       int32_t *state, int32_t *depth, double *reward, double *lower, double *upper, uint8_t *done,
                       int64_t *count, int32_t *first_child, int32_t *n_children);

/* ---------------------------------------------------------------- OLOP ---------------------- */
/*
 * OLOP.plan (tree_search/olop.py:94-100) for n_roots independent roots of a deterministic table model: `episodes` times
 * OLOP.run (:64-92) -- one generator draw (state.seed(np_random.randint(2**30)), :73), then exactly `horizon` model steps
 * (the reference does not stop at done): OLOPNode.expand (:165-180, the available actions in listing order) at a childless
 * node followed by the continuation action, else the first child of maximal value_upper (:84); OLOPNode.update (:132-142,
 * done sticky per node, reward range checked); compute_reward_ucb (:144-163); backup_to_root (:182-193) -- then get_plan
 * (abstract.py:143-156) with OLOPNode.selection_rule (:126-130).  Replaces the reference's per-episode safe_deepcopy_env.
 *   bound_type: 1 = "kullback-leibler" (kl_upper_bound, utils.py:123-203), anything else = mu_ucb stays inf (the reference
 *     logs "Unknown upper-bound type").
 *   continuation: < 0 = "uniform" (np_random.choice over the new children); >= 0 = the action label taken after an expansion
 *     ("zeros": action 0 of the environment); status MP_ERR_OLOP_KEY where it is not among the children.
 *   thresholds double [episodes]: the bound's threshold per episode (eval of the config string; read with bound_type 1 only).
 *   value_upper_init double [horizon + 1]: (1 - gamma ** (horizon + 1 - depth)) / (1 - gamma) by depth (olop.py:113).
 *   Both are host pointers: the host evaluates them with the reference's own Python operations.
 *   rng_state [n_roots][6], advanced; plans int32 [n_roots, max_plan_len] (-1 padded), plan_len, root_value = the root's
 *   value_upper, env_steps (= episodes * horizon without an error), status (MP_OK / MP_ERR_REWARD_RANGE / MP_ERR_OLOP_KEY).
 * The step limit of the model plays no part: the reference folds a step's 5-tuple with done = terminated.
 */
int mp_olop_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes, int32_t horizon,
                 double gamma, int32_t bound_type, int32_t continuation, const double *thresholds,
                 const double *value_upper_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len,
                 double *root_value, int64_t *env_steps, int32_t *status, int32_t mem);
/* Tree of root `root` after the last mp_olop_plan, in the reference's creation order (children contiguous, listing order):
 * per node parent (-1 at the root), action, depth, count, cumulative_reward, mu_ucb, value_upper, done, state (olop.py:102-116);
 * host arrays of capacity `cap` (at most 1 + episodes * horizon * |A| nodes).  When a batch's trees do not all fit the
 * workspace only root 0's is kept (MP_ERR_ARG for the others). */
int mp_olop_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *action,
                        int32_t *depth, int64_t *count, double *cumulative_reward, double *mu_ucb, double *value_upper,
                        uint8_t *done, int32_t *state);

/* mp_olop_plan on a batch model with one MDP per root (see mp_uct_plan_models): root i plans on MDP model_index[i] from its
 * LOCAL state root_state[i]; several roots may share an MDP.  Everything else as mp_olop_plan, and equal to it with
 * root_state = model_index * S_each + root_state; validation, MP_MEM_HOST / MP_MEM_DEVICE and the clamp-and-count of
 * out-of-range device arrays as mp_opd_plan_models; MP_ERR_MODE for a model that is not a deterministic table.  Replaces what
 * mp_olop_plan replaces (olop.py:64-100, the per-episode safe_deepcopy_env of :72) for a batch of agents that each hold their
 * own environment (trainer/evaluation.py:139-194, one process each).  The kernel either reads the batch model's records from
 * global memory ("olop_each_global") or copies the root's own S_each * |A| records into LDS first ("olop_each_lds"):
 * mp_each_form_info.  Nodes store GLOBAL states, and mp_olop_tree_export serves the trees afterwards. */
int mp_olop_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                        int32_t episodes, int32_t horizon, double gamma, int32_t bound_type, int32_t continuation,
                        const double *thresholds, const double *value_upper_init, uint64_t *rng_state, int32_t max_plan_len,
                        int32_t *plans, int32_t *plan_len, double *root_value, int64_t *env_steps, int32_t *status, int32_t mem);

/* OLOP.plan (tree_search/olop.py:64-193, utils.py:89-203) on a STOCHASTIC finite MDP: a whole dense ([S,A,S]) or sparse
 * ([S,A,B]) model.  Arguments, host tables, mem flags, validation and outputs are those of mp_olop_plan; what differs is what
 * the reference does on such an env:
 *   - run (:64-92) re-seeds its clone per episode, state.seed(np_random.randint(2**30)) (:73): the one draw x of the planner's
 *     generator makes the clone's Generator(PCG64(SeedSequence(x))), and every model step takes ONE double from THAT generator
 *     (k = next64 >> 11, successor #{j : thr_j <= k} over the row's thresholds ceil(cdf * 2^53)); reward R[s,a]; done by the
 *     model's done rule on the source or the next state (mp_model_set_episode_rules).  Exactly `horizon` steps, done or not;
 *   - the state belongs to the episode, not to the node: OLOPNode.expand (:165-180) lists the actions of the clone's CURRENT
 *     state (mp_model_set_available's row in column order, else every action), a node's children are fixed at its first
 *     expansion, and a later episode that reaches the node in another state steps the selected child (:84-88) whether or not
 *     that state lists its action;
 *   - OLOPNode.update (:132-142): the reward range is checked after the step was counted, done is sticky PER NODE (set by any
 *     realisation that reports it), a done node adds 0; compute_reward_ucb (:144-163), backup_to_root (:182-193) and get_plan
 *     with selection_rule (:126-130) as mp_olop_plan.
 * The planner's generator sees exactly the draws it sees on a table.  MP_ERR_MODE for a deterministic table (mp_olop_plan plans
 * on those) and for a joint, batch or row-block model.  mp_olop_tree_export serves the trees afterwards, same layout, creation
 * order and capacity; `state` holds the root's state at node 0 and -1 elsewhere (a node stands for no single state).
 * mp_last_kernel_variant records one of mp_olop_stoch_form_names: "olop_stoch_dense\nolop_stoch_sparse" (part of no other list). */
int mp_olop_plan_stochastic(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes,
                            int32_t horizon, double gamma, int32_t bound_type, int32_t continuation, const double *thresholds,
                            const double *value_upper_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                            int32_t *plan_len, double *root_value, int64_t *env_steps, int32_t *status, int32_t mem);
const char *mp_olop_stoch_form_names(void);

/* Test hook: what the DEVICE computes for the three functions behind mu_ucb, the only planner outputs that are held to a
 * tolerance (1e-12) and not to bits.  Host arrays of n elements in and out, one input per lane of 64-lane workgroups (the lanes
 * of a wave run different iteration counts, as the path nodes of an episode do); the kernel calls the very __device__ functions
 * olop_kernel calls.
 *   what 0: out[i] = kl_upper_bound(x[i] = cumulative reward, count[i], y[i] = threshold) (utils.py:123-203), with
 *     iterations[i] = the Newton iterations run and decisions[i] = the branches taken, as a bit mask: 1 = the in-loop upper
 *     clamp (utils.py:195), 2 = the in-loop lower clamp (:193), 4 = the finite difference that replaces the derivative after a
 *     ZeroDivisionError (:188), 8 / 16 = the final lower / upper clamp (:198-201);
 *   what 1: out[i] = bernoulli_kullback_leibler(p = x[i], q = y[i]) (utils.py:89-107);
 *   what 2: out[i] = log(x[i]), the device's;
 *   what 3: kl_upper_bound(..., lower=True) (utils.py:136-147, MDP-GapE's mu_lcb): inputs and outputs as what 0.
 * count, iterations and decisions are read and written with what 0 and 3 only; y with what 0, 1 and 3. */
int mp_selftest_olop_bound(mp_ctx *ctx, int32_t what, int32_t n, const double *x, const double *y, const int32_t *count,
                           double *out, int32_t *iterations, int32_t *decisions);

/* ---------------------------------------------------------------- MDP-GapE ------------------ */
/*
 * MDPGapE.plan (tree_search/mdp_gape.py:94-110) for n_roots independent roots of a deterministic table model, with
 * max_next_states_count 1: episodes of MDPGapE.run (:60-92) until challenger.value_upper - best.value_lower < accuracy or
 * episodes + 2 of them have run.  An episode: one generator draw (randint(2**30), :67); the root expanded if childless; exactly
 * `horizon` steps -- at the root the arm best_arm_identification_selection picks (:228-249), at an inner node with children
 * random_argmax over the chance children's value_upper (exact ties, a draw only for two or more), at a childless node
 * randint(n_actions_env) over ALL environment actions or action 0, an unlisted action giving way to the first listed one
 * (:155-160); ChanceNode.update, OLOPNode.update (olop.py:132-142: reward range, done sticky per node); then mu_ucb and mu_lcb
 * (kl_upper_bound, lower=False / True) of the path's decision nodes and backup_to_root (:214-226, :288-305; with one next state a
 * chance node's values are mu + gamma * value of its decision child).  get_plan: the best arm's action.
 *   continuation: 1 = "uniform", 0 = action 0 of the environment.
 *   action_column int32 [n_actions_env]: the model column of each environment action, -1 for none (NULL: the identity, and
 *     n_actions_env must equal |A|): the model's columns are in the environment's listing order.
 *   thr_by_count double [episodes + 2]: the bound's threshold for a node of count c at [c - 1] (eval of the config string);
 *   value_init double [horizon + 1]: (1 - gamma ** (horizon - depth)) / (1 - gamma).  Host pointers, evaluated in Python.
 *   rng_state [n_roots][6], advanced; plans int32 [n_roots, max_plan_len] (one action, -1 padded), plan_len, episodes_run,
 *   env_steps (= episodes_run * horizon without an error), status (MP_OK / MP_ERR_REWARD_RANGE / MP_ERR_GAPE_NO_CHALLENGER, or
 *   MP_ERR_ARG where a bound below the root came out NaN and random_argmax's tie set is empty: np_random.choice raises),
 *   child_lower / child_upper double and child_count int64 [n_roots, |A|]: the root's chance children by column (count -1
 *   where the root lists no such action), best_challenger int32 [n_roots, 2]: the actions of the two arms of the last episode.
 * MP_ERR_MODE for a dense, sparse, joint, batch or row-block model; MP_ERR_ARG, with the reason, for a gamma, accuracy,
 * threshold or initial value that is not finite (the reference plans on the NaN bounds they make) and when the node bound
 * 1 + (episodes + 2) * horizon * |A| does not fit a 32-bit index or 1 GiB.  mp_last_kernel_variant records one of
 * mp_gape_form_names: "gape_global\ngape_global_slots" (part of no other list).
 */
int mp_gape_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes, int32_t horizon,
                 double gamma, double accuracy, int32_t continuation, int32_t n_actions_env, const int32_t *action_column,
                 const double *thr_by_count, const double *value_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                 int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps, int32_t *status, double *child_lower,
                 double *child_upper, int64_t *child_count, int32_t *best_challenger, int32_t mem);
const char *mp_gape_form_names(void);
/* Tree of root `root` after the last mp_gape_plan, decision and chance nodes in the reference's creation order: per node its
 * kind (0 decision, 1 chance), parent (-1 at the root), action (a chance node's action column; a decision node's observed
 * state), depth (a chance node has its parent's), count, and cumulative_reward, mu_ucb, mu_lcb, done (0 for chance nodes, which
 * hold none), value_upper, value_lower, state.  Host arrays of capacity `cap` (at most 2 * (1 + (episodes + 2) * horizon * |A|)
 * nodes; *n_nodes is set also when `cap` is too small).  When a batch's trees do not all fit the workspace only root 0's is
 * kept (MP_ERR_ARG for the others).  The tree of a root whose status is not MP_OK is what the plan had built when it stopped,
 * not the reference's state at its raise (the failing step's counts and decision child are not booked). */
int mp_gape_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, uint8_t *kind, int32_t *parent, int32_t *action,
                        int32_t *depth, int64_t *count, double *cumulative_reward, double *mu_ucb, double *mu_lcb,
                        double *value_upper, double *value_lower, uint8_t *done, int32_t *state);

/* mp_gape_plan on a batch model of deterministic tables (mp_model_load_table_batch) with one MDP per root (see
 * mp_olop_plan_models / mp_ss_plan_models): model_index int32 [n_roots], root_state LOCAL; several roots may share an MDP.
 * Equal to MDPGapE.plan (tree_search/mdp_gape.py:94-110; the episodes of :60-92, the sampling rule of :185-196, the expansion
 * of :155-170, the bounds of :200-210, the backup of :214-226 and :288-305, best-arm identification of :228-249) of one agent
 * per MDP, and to mp_gape_plan on that table alone, bit for bit: every result, the generator records and every tree array.
 * The availability table is read as mp_gape_plan reads it: mp_model_set_available, one row per GLOBAL state, so every MDP
 * may list other actions; the done rule is the model's.  The remaining arguments and the results are mp_gape_plan's.
 * MP_ERR_MODE for a single table, a joint batch, a dense, a sparse or a row-block model; MP_ERR_ARG for a model_index outside
 * [0, N) or a local state outside [0, S_each) in host arrays (device arrays: the clamp-and-count of mp_opd_plan_models), and
 * under the conditions of mp_gape_plan.  This entry accepts batch models (mp_gape_plan itself refuses them).  Nodes hold
 * GLOBAL states: mp_gape_tree_export serves the trees afterwards, its `state` column (and a decision node's `action`) global.
 * mp_last_kernel_variant records one of mp_gape_each_form_names: "gape_each_lds" (the root's S_each * |A| records in LDS behind
 * path[horizon + 1]) / "gape_each_global", each also with "_slots" (part of no other list). */
int mp_gape_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                        int32_t episodes, int32_t horizon, double gamma, double accuracy, int32_t continuation,
                        int32_t n_actions_env, const int32_t *action_column, const double *thr_by_count, const double *value_init,
                        uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len, int32_t *episodes_run,
                        int64_t *env_steps, int32_t *status, double *child_lower, double *child_upper, int64_t *child_count,
                        int32_t *best_challenger, int32_t mem);
const char *mp_gape_each_form_names(void);
/* The form mp_gape_plan_models chooses for a call of this description, on the host alone (no device, no ctx; the function the
 * launch code calls), with the six outputs of mp_each_form_info: the kernel's own LDS array is path[horizon + 1] int32, as
 * OLOP's.  The LDS form is the default where it was measured faster beyond the spread of repeated medians (each_host.hpp): a
 * workgroup of at most 160 KiB / 16 bytes, from 256 roots on, while all the roots' workgroups are resident at once; else the global
 * form.  MP_EACH_MODEL=lds takes the LDS form for any table that fits the 160 KiB of a CU, MP_EACH_MODEL=global the global one. */
int mp_gape_each_form_info(int32_t S_each, int32_t A, int32_t horizon, int32_t n_roots, int32_t cus, int64_t *out);

/*
 * MDPGapE.plan with a KL confidence region over every chance node's next-state distribution: max_next_states_count =
 * max_next_states in 1..32, on a deterministic table, a dense or a sparse model.  Everything mp_gape_plan does, and:
 *   - the clone is re-seeded per episode from the planner's draw (mdp_gape.py:67): Generator(PCG64(SeedSequence(x))), and a step
 *     of a dense / sparse model draws one double of it (a deterministic table draws nothing).  A decision node stands for one
 *     observed state and lists that state's actions (:162-170);
 *   - a chance node gets max_next_states placeholder decision children at its first get_child (:267-270: mu_ucb 1, mu_lcb 0,
 *     value_upper the initial value of depth + 1, value_lower 0); a state not seen before takes the lowest placeholder left
 *     (:277-282), and status MP_ERR_GAPE_PLACEHOLDERS where none is left (:284-285 ValueError), after the step was counted;
 *   - a chance node's backup (:288-305): over its children in the reference's dict order -- the placeholders left, then the
 *     observed states by first observation -- u_next = mu_ucb + gamma * value_upper, l_next = mu_lcb + gamma * value_lower,
 *     p_hat = count / the node's count, threshold = transition_thr_by_count[count - 1] / count; value_upper = p_plus @ u_next
 *     and value_lower = p_minus @ l_next for p_plus = max_expectation_under_constraint(u_next, p_hat, threshold) and
 *     p_minus = (-l_next, p_hat, threshold) (utils.py:292-342 with newton_iteration :150-203), every branch with numpy's
 *     semantics.  The two solves run side by side in the halves of the wavefront.
 *   transition_thr_by_count double [episodes + 2]: transition_threshold() (:307-313) for a chance node of count c at [c - 1].
 * Results as mp_gape_plan.  MP_ERR_MODE for a CartPole, joint, batch or row-block model; MP_ERR_ARG for max_next_states outside
 * 1..32, for a gamma, accuracy, threshold of either table or initial value that is not finite, and when the node bound
 * 1 + (episodes + 2) * horizon * max_next_states + (1 + (episodes + 2) * horizon) * |A| does not fit a 32-bit index or 1 GiB.
 * At max_next_states 1 on a deterministic table every result equals mp_gape_plan's bit for bit.  mp_last_kernel_variant records
 * one of mp_gape_stoch_form_names: "gape_stoch_{table,dense,sparse}[_slots]" (part of no other list).
 */
int mp_gape_plan_stochastic(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t episodes,
                            int32_t horizon, int32_t max_next_states, double gamma, double accuracy, int32_t continuation,
                            int32_t n_actions_env, const int32_t *action_column, const double *thr_by_count,
                            const double *transition_thr_by_count, const double *value_init, uint64_t *rng_state,
                            int32_t max_plan_len, int32_t *plans, int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps,
                            int32_t *status, double *child_lower, double *child_upper, int64_t *child_count,
                            int32_t *best_challenger, int32_t mem);
const char *mp_gape_stoch_form_names(void);
/* mp_gape_plan_stochastic on a batch model of deterministic tables (mp_model_load_table_batch) with one MDP per root (see
 * mp_gape_plan_models): model_index int32 [n_roots], root_state LOCAL; several roots may share an MDP.  After model_index the
 * arguments and the results are mp_gape_plan_stochastic's.  Equal to MDPGapE.plan (tree_search/mdp_gape.py:94-110 with
 * max_next_states_count = max_next_states in 1..32) of one agent per MDP, and to mp_gape_plan_stochastic on that table alone, bit
 * for bit: every result, the generator records and every array of the exported tree; at max_next_states 1 also to
 * mp_gape_plan_models.  The availability table is read per GLOBAL state (mp_model_set_available), so every MDP may list other
 * actions; the done rule is the model's.  MP_ERR_MODE for a single table, a dense, sparse, joint, joint-batch or row-block model
 * (mp_gape_plan_stochastic itself keeps refusing batch models); MP_ERR_ARG for a model_index outside [0, N) or a local state
 * outside [0, S_each) in host arrays (device arrays: the clamp-and-count of mp_opd_plan_models), and under the conditions of
 * mp_gape_plan_stochastic.  Nodes hold GLOBAL states: mp_gape_stoch_tree_export serves the trees afterwards, its `state` column
 * (and a decision node's `action`) global.  mp_last_kernel_variant records one of mp_gape_stoch_each_form_names:
 * "gape_stoch_each_lds" (the root's S_each * |A| records in LDS behind path[2 * horizon + 1]) / "gape_stoch_each_global", each
 * also with "_slots" (part of no other list). */
int mp_gape_plan_stochastic_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index,
                                   const int32_t *root_state, int32_t episodes, int32_t horizon, int32_t max_next_states,
                                   double gamma, double accuracy, int32_t continuation, int32_t n_actions_env,
                                   const int32_t *action_column, const double *thr_by_count, const double *transition_thr_by_count,
                                   const double *value_init, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                                   int32_t *plan_len, int32_t *episodes_run, int64_t *env_steps, int32_t *status,
                                   double *child_lower, double *child_upper, int64_t *child_count, int32_t *best_challenger,
                                   int32_t mem);
const char *mp_gape_stoch_each_form_names(void);
/* The form mp_gape_plan_stochastic_models chooses for a call of this description, on the host alone (no device, no ctx; the
 * function the launch code calls), with the six outputs of mp_gape_each_form_info: the kernel's own LDS array is
 * path[2 * horizon + 1] int32, 16-byte rounded.  The LDS form is the default where it was measured faster beyond the spread of
 * repeated medians (each_host.hpp), which is where mp_gape_plan_models has it: a workgroup of at most 160 KiB / 16 bytes, from
 * 256 roots on, while all the roots' workgroups are resident at once; else the global form.  MP_EACH_MODEL=lds takes the LDS
 * form for any table that fits the 160 KiB of a CU, MP_EACH_MODEL=global the global one. */
int mp_gape_stoch_each_form_info(int32_t S_each, int32_t A, int32_t horizon, int32_t n_roots, int32_t cus, int64_t *out);
/* Tree of root `root` after the last mp_gape_plan_stochastic, BREADTH FIRST over decision and chance nodes, a node's children in
 * the reference's dict order (a chance node's: the placeholders left in number order, then the observed states by first
 * observation, mdp_gape.py:281).  The fields of mp_gape_tree_export; `parent` is a position of this listing; the action of a
 * decision node is its observed state, or -1 - i for placeholder_i (state -1).  At most the node bound of the plan call; *n_nodes
 * is set also when `cap` is too small.  The tree of a root whose status is not MP_OK is what the plan had built when it stopped. */
int mp_gape_stoch_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, uint8_t *kind, int32_t *parent,
                              int32_t *action, int32_t *depth, int64_t *count, double *cumulative_reward, double *mu_ucb,
                              double *mu_lcb, double *value_upper, double *value_lower, uint8_t *done, int32_t *state);
/* What the DEVICE computes for max_expectation_under_constraint (utils.py:292-342; csrc/kl_transition.hpp) on n problems of
 * width K in 1..32, two problems per wavefront as in the planner: f, q double [n][K], c double [n] -> p_star double [n][K], the
 * Newton iterations and the decisions taken (the KT_* bits of kl_transition.hpp) int32 [n].  Host arrays. */
int mp_selftest_gape_transition(mp_ctx *ctx, int32_t n, int32_t K, const double *f, const double *q, const double *c,
                                double *p_star, int32_t *iterations, int32_t *decisions);

/* ---------------------------------------------------------------- BRUE ---------------------- */
/*
 * BRUE.plan (tree_search/brue.py:66-71) for n_roots independent roots of a deterministic table, dense or sparse model: while
 * the budget lasts, one rollout (:24-33) -- one generator draw state.seed(np_random.randint(2**30)) (:25, made for every
 * model), then up to `horizon` steps of a uniformly random action (np_random.randint(|A|), :27: every action, whatever the
 * env lists as available), each spending one unit of budget, until a step reports done (= terminated, by the model's done
 * rule; the step limit plays no part) -- and `update` (:35-50): DecisionNode / ChanceNode.get_child (:93-96, :113-116,
 * children in creation order), then from the last step up the running means of DecisionNode.update (:84-86) and
 * ChanceNode.update (:106-108) on reward + gamma * estimate(next) (:52-64: the first chance child of maximal value, an outcome
 * drawn with np_random.choice(..., p=counts / counts.sum()), one double even for a single child).  A dense / sparse model's
 * step draws one double from the clone's own generator, Generator(PCG64(SeedSequence(x))) of the rollout's 30-bit draw x
 * (FiniteMDPEnv.seed); a deterministic table draws nothing.  Then get_plan (:73-75): DecisionNode.selection_rule (:88-91),
 * Node.random_argmax (abstract.py:296-311) over the root's chance children.  Replaces the reference's per-rollout
 * safe_deepcopy_env.  Bit-exact with the reference (+ - * / on f64, integer counts).
 *   gpow double [horizon + 1]: gamma ** d (a host pointer: the host's Python `**`).  1 <= horizon <= 4096.
 *   rng_state [n_roots][6], advanced; plans int32 [n_roots] the ONE planned action (-1: no rollout was made, budget <= 0 --
 *   the reference raises ValueError from np.amax([])); root_value = the value of the chosen chance child; env_steps = model
 *   steps taken (the last rollout may overshoot the budget); status MP_OK.
 * An availability table on the model (mp_model_set_available) is not read: BRUE draws among all actions (:27).
 */
int mp_brue_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t budget, int32_t horizon,
                 double gamma, const double *gpow, uint64_t *rng_state, int32_t *plans, double *root_value, int64_t *env_steps,
                 int32_t *status, int32_t mem);
/* Tree of root `root` after the last mp_brue_plan, in the reference's creation order: per node parent (-1 at the root), key
 * (the action of a chance node, the observed state of a decision node, -1 at the root), is_chance, depth (brue.py:81,103),
 * count, stat (DecisionNode.reward / ChanceNode.value); host arrays of capacity `cap` (at most 1 + 2 * (budget + horizon)
 * nodes).  When a batch's trees do not all fit the workspace only root 0's is kept (MP_ERR_ARG for the others). */
int mp_brue_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *key,
                        uint8_t *is_chance, int32_t *depth, int64_t *count, double *stat);

/* mp_brue_plan on a batch model of deterministic tables with one MDP per root (see mp_uct_plan_models / mp_olop_plan_models):
 * model_index int32 [n_roots], root_state LOCAL; equal to BRUE.plan (brue.py:66-71, the per-rollout safe_deepcopy_env of :24)
 * of one agent per MDP.  This entry accepts batch models (mp_brue_plan itself refuses them); MP_ERR_MODE for a dense / sparse
 * or joint model.  Decision nodes' keys are GLOBAL states; mp_brue_tree_export serves the trees afterwards.  Forms
 * "brue_each_global" / "brue_each_lds": mp_each_form_info. */
int mp_brue_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                        int32_t budget, int32_t horizon, double gamma, const double *gpow, uint64_t *rng_state, int32_t *plans,
                        double *root_value, int64_t *env_steps, int32_t *status, int32_t mem);
/* The form mp_olop_plan_models (planner 0) / mp_brue_plan_models (planner 1) / mp_ss_plan_models (planner 2) choose for a call of this description, on the host
 * alone (no device, no ctx; the function the launch code calls).  A root of these calls reads only its own MDP -- the
 * reference's agent only its own env (olop.py:72, brue.py:24) -- so its S_each * |A| 16-byte records can sit in LDS behind the
 * kernel's own arrays (OLOP: path[horizon + 1] int32; BRUE: 16 bytes per step of the horizon; Sparse Sampling: a frame of 64
 * bytes per level of the horizon; rounded up to 16 bytes).
 * The LDS form is the default where it was measured faster: a workgroup of at most 160 KiB / 16 bytes (16 wavefronts stay
 * resident on a CU); OLOP at any batch size, BRUE and Sparse Sampling while all their roots' workgroups are resident at once.  MP_EACH_MODEL=lds|global
 * in the environment forces a form ("lds" for any table that fits the 160 KiB of a CU, and only those).
 *   out[6]: LDS bytes a workgroup of the LDS form takes (the arrays + S_each * |A| * 16), 1 if this call takes the LDS form else
 *           0, the grid = min(n_roots, cus * min(32, floor(160 KiB / those bytes))) of the LDS form, min(n_roots, cus * 32) of the
 *           global form, dynamic LDS bytes of the launch, the most bytes that take the LDS form by default, the most that fit. */
int mp_each_form_info(int32_t planner, int32_t S_each, int32_t A, int32_t horizon, int32_t n_roots, int32_t cus, int64_t *out);
/* The eight names the two entries above record for mp_last_kernel_variant, one per line: "olop_each_lds", "olop_each_global",
 * "brue_each_lds", "brue_each_global", each also with "_slots" (see mp_last_kernel_variant).  They are not part of
 * mp_kernel_form_names. */
const char *mp_each_form_names(void);

/* ---------------------------------------------------------------- Sparse Sampling ----------- */
/*
 * SparseSampling.plan (tree_search/sparse_sampling.py:21-24) for n_roots independent roots of a deterministic table, dense or
 * sparse model: DecisionNode.estimateV (:38-51) visits the actions the env lists (the model's availability table, in column
 * order; every action without one), ChanceNode.estimateQ (:71-88) takes C samples -- each one generator draw
 * np_random.randint(2**30) (:79, made for every model kind), a clone seeded with it, Generator(PCG64(SeedSequence(x))), and one
 * step, which draws one double on a dense / sparse model and nothing on a table -- lists the outcomes in first-occurrence
 * order with their counts (:83, :93-96), recurses into them in that order down to depth `horizon` and backs up
 * reward + gamma * sum(value * count) / C (:87-88) with the LAST sample's reward; `done` is never read (:81).  Then get_plan
 * (:26-28): DecisionNode.selection_rule (:53-56), Node.random_argmax (abstract.py:296-311) over the root's chance children.
 * Replaces the reference's per-sample safe_deepcopy_env.  Bit-exact with the reference (+ * / on f64, integer counts).
 *   1 <= horizon <= 16, 1 <= C <= 1024 (else MP_ERR_ARG; the reference raises ValueError at horizon 0 and UnboundLocalError
 *   at C 0); MP_ERR_ARG too for a tree whose node bound -- D_0 = 1 decision node, |A| D_d chance nodes at depth d,
 *   D_(d+1) <= |A| D_d min(C, W), W the most outcomes one (state, action) can give -- exceeds int32 indices or the workspace.
 *   MP_ERR_MODE for joint, batch and row-block models.
 *   rng_state [n_roots][6], advanced; plans int32 [n_roots] the ONE planned action (a column of the model); root_value = the
 *   value of the chosen chance child; samples = model steps taken (the reference's own step count, len(planner.observations),
 *   stays 0: the samples step the clone directly); status MP_OK.
 * The frames of the recursion sit in LDS ("ss_wave_lds") or, when horizon * min(C, W) list entries exceed 16 KiB, in a global
 * workspace ("ss_wave_global"); MP_SS_FRAMES=lds|global in the environment forces either where it is legal.
 */
int mp_ss_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t horizon, int32_t C, double gamma,
               uint64_t *rng_state, int32_t *plans, double *root_value, int64_t *samples, int32_t *status, int32_t mem);
/* Tree of root `root` after the last call of the plan above, in the reference's creation order: per node parent (-1 at the
 * root), key (the action of a chance node, the observed state of a decision node, -1 at the root), is_chance, depth
 * (sparse_sampling.py:34,68), count (:83; 0 for chance nodes), value (:51, :87; the int 0 of a node at depth `horizon` is 0.0);
 * host arrays of capacity `cap` (*n_nodes is set even when `cap` is too small).  Trees are kept for every root while the
 * batch's node bounds fit the workspace (1 GiB, or MP_SS_KEEP_BYTES if smaller), else only root 0's (MP_ERR_ARG for the others). */
int mp_ss_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *key, uint8_t *is_chance,
                      int32_t *depth, int64_t *count, double *value);
/* Host arithmetic of the plan above (no device): out[5] = { L = min(C, W) entries of an outcome list, bytes of a wave's frames,
 * the node bound of a tree (-1: beyond int32), the most frame bytes kept in LDS by default, 1 if this call's frames go to LDS
 * (MP_SS_FRAMES is read) else 0 }. */
int mp_ss_geometry(int32_t n_actions, int32_t horizon, int32_t C, int32_t W, int64_t *out);
/* The two names the plan above records for mp_last_kernel_variant, one per line (they are not part of mp_kernel_form_names). */
const char *mp_ss_form_names(void);

/* mp_ss_plan on a batch model of deterministic tables with one MDP per root (see mp_opd_plan_models / mp_brue_plan_models):
 * model_index int32 [n_roots], root_state LOCAL; several roots may share an MDP.  Equal to SparseSampling.plan
 * (sparse_sampling.py:21-28; the per-sample safe_deepcopy_env of :80 and the recursion of :38-51 / :71-88) of one agent per
 * MDP, and to mp_ss_plan on that table alone, bit for bit: plans, root values, samples, generator records and every tree
 * array.  The availability table is read as mp_ss_plan reads it: mp_model_set_available, one row per GLOBAL state.
 * Validation, MP_MEM_HOST / MP_MEM_DEVICE and the clamp-and-count of out-of-range device arrays as mp_opd_plan_models;
 * MP_ERR_MODE for a dense, sparse, joint or row-block model; MP_ERR_ARG under the conditions of mp_ss_plan (horizon, C, node
 * bound).  This entry accepts batch models (mp_ss_plan itself refuses them).  Decision nodes' keys are GLOBAL states;
 * mp_ss_tree_export serves the trees afterwards, under the same keep rule.
 * On a table an outcome list has one entry: a frame is 64 bytes, the frames always sit in LDS and MP_SS_FRAMES is not read.
 * Forms "ss_each_global" / "ss_each_lds" (the root's S_each * |A| records in LDS behind the frames): mp_each_form_info,
 * planner 2. */
int mp_ss_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                      int32_t horizon, int32_t C, double gamma, uint64_t *rng_state, int32_t *plans, double *root_value,
                      int64_t *samples, int32_t *status, int32_t mem);
/* The names the entry above records for mp_last_kernel_variant, one per line (part of neither mp_kernel_form_names,
 * mp_each_form_names nor mp_ss_form_names). */
const char *mp_ss_each_form_names(void);

/* ---------------------------------------------------------------- discrete robust OPD ------- */
/*
 * A joint environment of M models of one decision problem stepped together (agents/robust/robust.py:9-26 JointEnv): the
 * planner's clone is the M state indices, a step returns M rewards and M terminal flags.
 *   transition int64 [M,S,A], reward double [M,S,A], terminal uint8 [M,S] or NULL (each model has its own flags).
 * The model is also a table model (M models) for the other entry points, which use model 0 for tree search.
 */
int mp_model_load_joint(mp_ctx *ctx, int32_t M, int32_t S, int32_t A, const int64_t *transition, const double *reward,
                        const uint8_t *terminal, int32_t done_on_next, mp_model **out);
/*
 * Models that restrict their available actions: JointEnv.get_available_actions (robust.py:22-25) lists, for a joint
 * state, the UNION of what each model's env lists in its own state (a model without get_available_actions lists every
 * action); DeterministicNode.expand (deterministic.py:32-35) creates one child per listed action.
 *   available uint8 [M,S,A], host pointer; every (model, state) needs at least one action.  A tree node has
 *   n_children <= A children (mp_ropd_tree_export), env_steps counts one joint step per real child.
 */
int mp_model_set_available_joint(mp_model *model, const uint8_t *available);
/*
 * DiscreteRobustPlanner.plan (agents/robust/robust.py:28-40 over tree_search/deterministic.py:116-122) for n_roots
 * independent roots of a joint model: budget // A times { leaf = first maximal min_m U among the leaves (robust.py:37,
 * RobustNode.get_value_upper_bound :45-46); DeterministicNode.expand (deterministic.py:28-43) with the ndarray branch of
 * update (:45-65): per-model lower / upper bounds; backup_to_root (:74-79) on the minima over the models }, then get_plan
 * with selection_rule (:21-26) on min_m L.  Rewards outside [0,1] in ANY model: status MP_ERR_REWARD_RANGE.
 *   root_state int32 [n_roots,M] (usually the same state M times); root_lower / root_upper = min over the models of
 *   the root's bounds; everything else as mp_opd_plan.  Any number of models (the reference steps a list, robust.py:9-16).
 */
int mp_ropd_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *root_state, int32_t budget, double gamma,
                 double terminal_reward, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len,
                 double *root_lower, double *root_upper, int64_t *env_steps, int32_t *status, int32_t mem);
/*
 * One SET of M models per root.  DiscreteRobustPlannerAgent.plan builds its models again before every plan --
 * preprocess_env(self.true_env, preprocessors) for each entry of config["models"], the M results in a JointEnv
 * (agents/robust/robust.py:68-71) -- so a batch of such agents on environments whose tables are extracted at every step holds
 * N sets of M hypothesis tables, all of which change between two steps.
 *   transition int64 [N,M,S,A] (next states LOCAL to each table, 0 <= t < S), reward double [N,M,S,A],
 *   terminal uint8 [N,M,S] or NULL; done_on_next as mp_model_load_joint.  N * S * A < 2^31, and the N * M * S * A records
 *   (with their tables, 28 bytes each) must fit the device's memory: else MP_ERR_ARG.
 * The result is ONE joint model of M models over the disjoint union of the N state spaces: GLOBAL state n * S + s, the
 * records model-major over global states ([M][N * S][A], next states global), mp_model_info reports M and S = N * S,
 * mp_model_batch_info N and S.  mp_ropd_plan takes it with global joint states, mp_ropd_plan_models with (set, local joint
 * state) pairs; the kernels are those of a plain joint model.  Tree exports report global states.
 */
int mp_model_load_joint_batch(mp_ctx *ctx, int32_t N, int32_t M, int32_t S, int32_t A, const int64_t *transition,
                              const double *reward, const uint8_t *terminal, int32_t done_on_next, mp_model **out);
/*
 * Replace sets [first, first + count) of such a model: the per-step delta of a batch of robust agents (robust.py:68-71 once
 * per agent and step).  Arrays as mp_model_load_joint_batch with N = count (host pointers; terminal iff the model was loaded
 * with terminal flags).  Availability flags set before are kept.  A next state outside [0, S) returns MP_ERR_ARG and leaves
 * the model as it was.  Stream-ordered through the model's pinned staging block like mp_model_update_tables; ONE launch packs
 * the count * M tables.  (mp_model_update_tables / _rows refuse every joint model, this one included: MP_ERR_MODE.)
 */
int mp_model_update_joint_tables(mp_model *model, int32_t first, int32_t count, const int64_t *transition, const double *reward,
                                 const uint8_t *terminal);
/*
 * JointEnv.get_available_actions (robust.py:22-25) for every set: available uint8 [N,M,S,A], host pointer; every
 * (set, model, state) needs at least one action.  The flags live in the records (the union over the models is taken by the
 * planner per joint state) and survive mp_model_update_joint_tables.
 */
int mp_model_set_available_joint_batch(mp_model *model, const uint8_t *available);
/*
 * mp_ropd_plan with one set per root (robust.py:68-73: every agent plans on the joint env it has just built): root i plans on
 * set model_index[i] from the LOCAL joint state root_state[i][0..M).
 *   model_index int32 [n_roots], root_state int32 [n_roots,M]; everything else as mp_ropd_plan (MP_MEM_HOST, MP_MEM_DEVICE,
 *   MP_MEM_RNG_DEVICE).  Host arrays out of range: MP_ERR_ARG; device arrays: the root is clamped to state 0 of set 0 and
 *   counted (mp_ctx_device_faults), as mp_opd_plan_models does.  MP_ERR_MODE for anything but a model of
 *   mp_model_load_joint_batch.  The kernel is mp_ropd_plan's, and so is the name mp_last_kernel_variant reports.
 */
int mp_ropd_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                        int32_t budget, double gamma, double terminal_reward, uint64_t *rng_state, int32_t max_plan_len,
                        int32_t *plans, int32_t *plan_len, double *root_lower, double *root_upper, int64_t *env_steps,
                        int32_t *status, int32_t mem);
/* Tree of root `root` after the last mp_ropd_plan / mp_ropd_plan_models, creation order (A children per expanded node); host arrays of capacity
 * `cap` nodes; state / reward / lower / upper / done are [cap,M]: a leaf's per-model values, an expanded node's
 * backed-up scalars repeated M times; n_children: children per node (contiguous from first_child; < A with restricted
 * action sets). */
int mp_ropd_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *action,
                        int32_t *state, int32_t *depth, double *reward, double *lower, double *upper, uint8_t *done,
                        int64_t *count, int32_t *first_child, int32_t *n_children);

/* ---------------------------------------------------------------- state-aware OPD ----------- */
/*
 * StateAwarePlanner / StateAwareNode (tree_search/state_aware.py:10-137) over DeterministicNode.expand/update
 * (deterministic.py:28-65): optimistic planning that aggregates the tree nodes observed in the same state.
 * An mp_saopd holds, for n_planners independent planners of one table model, what a reference planner OBJECT holds
 * across plan() calls: state_values and state_nodes (dictionaries keyed by str(observation) = the state index, :81-83)
 * and every node ever created -- reset() (deterministic.py:102-104) only installs a new root and leaves list, so nodes
 * of earlier trees keep taking part in prune() (:28-40) and backup_to_root() (:42-63) through state_nodes.
 * mp_saopd_plan = step_by_reset + StateAwarePlanner.plan (:117-127) for every planner:
 *   root_state int32 [n]; budget // |A| iterations of run() (:93-107); accuracy / backup_aggregated_nodes /
 *   prune_suboptimal_leaves = the config of default_config (:85-91); gamma must not change between plans.
 *   rng_state uint64 [n,6]: get_plan's random tie-breaks (deterministic.py:21-26), drawn twice per plan as the
 *   reference does (deterministic.py:122 + state_aware.py:127).
 *   plans int32 [n,max_plan_len] (-1 padded), plan_len int32 [n], env_steps / updates int64 [n] (planner.step calls /
 *   Bellman backups of this plan), status int32 [n]: MP_OK, MP_ERR_REWARD_RANGE (ValueError, deterministic.py:46-47),
 *   MP_ERR_ARG (every leaf pruned: the reference's max() of an empty list, :95) or MP_ERR_ALLOC (backup queue full and
 *   no room to grow it: a full queue normally rolls the plan back and runs it again with a larger one).
 *   mem = MP_MEM_HOST: the call synchronises (it returns host arrays), reads the overflow flag and retries by itself.
 *   mem = MP_MEM_DEVICE: ASYNCHRONOUS, one launch and nothing read back; a planner whose queue fills up then reports
 *   MP_ERR_ALLOC in `status`, cannot be rolled back, and stays failed: every later call reports MP_ERR_ALLOC for it again
 *   (the other planners of the batch are unaffected).  The same holds for the planners left full when a host-mode call
 *   runs out of room to grow the queue.  A planner whose leaves were ALL pruned (the reference raises ValueError from
 *   max() there, state_aware.py:95) reports MP_ERR_ARG and, in the asynchronous mode -- where the caller goes on stepping
 *   the batch -- stays failed the same way.
 * The model must outlive the planners (they read its transition records).
 * mp_saopd_export: arena of one planner in creation order (node rows [root, n_nodes) are the current tree; `alive` =
 * "in planner.leaves"), arrays of capacity >= n_nodes (mp_saopd_info), and state_values double [S].
 * Restricted action sets (mp_model_set_available on the model; deterministic.py:32-35): an expansion still takes |A|
 * consecutive rows, the rows of unlisted actions are PHANTOMS -- lower = -inf, never alive, in no state's list, count 0 --
 * that a caller drops (rl_agents_amd/native.py StateAwarePlanners.export does, and renumbers); env_steps counts the
 * listed actions only.
 */
typedef struct mp_saopd mp_saopd;
int mp_saopd_create(mp_ctx *ctx, mp_model *model, int32_t n_planners, mp_saopd **out);
int mp_saopd_free(mp_saopd *planners);
int mp_saopd_plan(mp_ctx *ctx, mp_saopd *planners, const int32_t *root_state, int32_t budget, double gamma,
                  double terminal_reward, double accuracy, int32_t backup_aggregated_nodes,
                  int32_t prune_suboptimal_leaves, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                  int32_t *plan_len, int64_t *env_steps, int64_t *updates, int32_t *status, int32_t mem);
int mp_saopd_info(mp_saopd *planners, int32_t *n_planners, int32_t *n_nodes, int32_t *root, int32_t *n_states);
int mp_saopd_export(mp_saopd *planners, int32_t planner, int32_t cap, int32_t *parent, int32_t *action, int32_t *state,
                    int32_t *depth, double *reward, double *lower, uint8_t *done, int64_t *count, int32_t *first_child,
                    uint8_t *alive, double *state_values);

/* ---------------------------------------------------------------- GBOP-D -------------------- */
/*
 * GraphBasedPlanner / GraphNode (tree_search/graph_based.py:12-151): optimistic planning on the GRAPH of observed states
 * -- one node per state, a lower and an upper bound of V per node, tightened after every expansion by a partial value
 * iteration that runs backwards through the graph (a first-in-first-out queue with duplicates, :66-78).
 * An mp_gbopd handle holds, for n_planners independent planners of one deterministic table model (with or without an
 * availability table and listing order; any other model kind answers MP_ERR_MODE), what a reference planner OBJECT holds
 * across plan() calls: planner.nodes (bounds, children, parents), updates_count and observations -- reset() (:93-94) only
 * replaces `root`, so every later plan continues on the same graph.  queue_cap: entries of a planner's backup queue
 * (rounded up to a power of two; <= 0: MP_GBOPD_QUEUE in the environment, else 65 536, less for batches whose rings would
 * exceed 4 GiB: such a batch should name its capacity).
 * mp_gbopd_plan = GraphBasedPlanner.plan (:118-124) for every planner: root = get_node(root_state), budget // |A| epochs
 * of run() (:96-108; |A| is the model's action count), then get_plan (:126-135).
 *   value_max = 1 / (1 - gamma) as the host computes it (:18); accuracy and sampling_timeout as in the config (:148-149).
 *   -1 < gamma < 1 and accuracy >= 0 are required (MP_ERR_ARG): outside them the reference's queue never empties.
 *   rng_state uint64 [n,6]: the tie draws of sampling_rule (:22-30); a single maximum does not advance the generator.
 *   plans int32 [n,sampling_timeout] (-1 padded; actions are the model's slots = the listing order), plan_len int32 [n],
 *   value_lower / value_upper double [n] (the root's bounds), env_steps / updates int64 [n] (observations appended /
 *   queue pops of this call), status int32 [n]: MP_OK, MP_ERR_ALLOC (the planner's queue filled up: its graph is half
 *   updated and it stays failed -- every later call reports MP_ERR_ALLOC for it again; the other planners are unaffected)
 *   MP_ERR_ARG (root state out of range in a device array), MP_ERR_GBOPD_NO_ACTION (a node no action is listed for: the
 *   reference raises ValueError) or MP_ERR_GBOPD_DIVERGED (more than 2^22 pops in one plan: with accuracy 0 and rewards
 *   outside [0, 1] the bounds can cycle for ever and the reference never returns); a planner that reported either stays
 *   failed, as with MP_ERR_ALLOC.  Tables or action sets that changed under a kept graph (mp_model_update_tables / _rows,
 *   mp_model_set_available after mp_gbopd_create): mp_gbopd_plan and mp_gbopd_export RETURN MP_ERR_ARG with the reason.
 *   mem = MP_MEM_HOST synchronises; MP_MEM_DEVICE is one asynchronous launch on the context's stream.
 * The parents of a node are kept and appended in INSERTION order (the reference iterates a set hashed by address there).
 * mp_gbopd_export: one planner's graph in creation order, arrays of capacity cap >= n_nodes (at most n_states):
 *   state, lower, upper, expanded [cap]; child int32 / reward double [cap, n_actions]: per slot the creation index of the
 *   child (-1: not listed, or the node is not expanded) and its reward; parent_ptr int32 [cap + 1] and parent_idx int32
 *   [n_edges (mp_gbopd_info)]: the parents' creation indices in order; visits / updates int64 [n_states]: the lifetime
 *   counters by state (get_visits, abstract.py:163-167; get_updates); n_observations = len(planner.observations);
 *   root = creation index of the last root.
 * The model must outlive the planners and keep its tables.
 */
typedef struct mp_gbopd mp_gbopd;
int mp_gbopd_create(mp_ctx *ctx, mp_model *model, int32_t n_planners, int32_t queue_cap, mp_gbopd **out);
int mp_gbopd_free(mp_gbopd *planners);
int mp_gbopd_plan(mp_ctx *ctx, mp_gbopd *planners, const int32_t *root_state, int32_t budget, double gamma, double value_max,
                  double accuracy, int32_t sampling_timeout, uint64_t *rng_state, int32_t *plans, int32_t *plan_len,
                  double *value_lower, double *value_upper, int64_t *env_steps, int64_t *updates, int32_t *status, int32_t mem);
int mp_gbopd_info(mp_gbopd *planners, int32_t *n_planners, int32_t *n_states, int32_t *n_actions, int32_t *queue_cap,
                  int64_t *n_edges);
int mp_gbopd_export(mp_gbopd *planners, int32_t planner, int32_t cap, int32_t *n_nodes, int32_t *state, double *lower,
                    double *upper, uint8_t *expanded, int32_t *child, double *reward, int32_t *parent_ptr, int32_t *parent_idx,
                    int64_t *visits, int64_t *updates, int64_t *n_observations, int32_t *root);

/* ---------------------------------------------------------------- GBOP ---------------------- */
/*
 * StochasticGraphBasedPlanner / GraphDecisionNode / GraphChanceNode (tree_search/graph_based_stochastic.py:15-343): GBOP,
 * optimistic planning on the graph of observed states of a STOCHASTIC MDP, with known rewards and a KL confidence region over
 * every (state, action)'s next-state distribution.  It serves the configs whose reward threshold evaluates to 0 -- every
 * config the reference ships ("0*np.log(time)"): compute_reward_ucb then takes mu_ucb = mu_lcb = cumulative_reward / count
 * (:76-77).  Any other value reaches the mis-called kl_upper_bound (:79-82) and is reported as the reference's TypeError.
 * An mp_gbop handle holds, for n_planners independent planners of one finite MDP (mp_gbop_create replaces the planner's
 * constructor and what reset(), :339-343, leaves alone) -- a deterministic table, a dense or a sparse model, with or without an
 * availability table and listing order; CartPole, joint, batch and row-block models answer MP_ERR_MODE -- what a reference
 * planner OBJECT holds across plan() calls and agent.reset(): planner.nodes with both bounds, count and parents of every
 * state, and per (state, listed action) the chance node with its count, stored bounds, p_plus / p_minus and its
 * max_next_states (1..32, else MP_ERR_ARG) transition children: placeholder or observed state, count, cumulative reward,
 * mu_ucb, mu_lcb.  queue_cap as mp_gbopd_create (MP_GBOP_QUEUE in the environment).
 * mp_gbop_free replaces the planner object's end of life.
 * mp_gbop_plan = StochasticGraphBasedPlanner.plan (:332-337) for every planner: root = get_node(root_state), `episodes` calls
 * of run() (:234-268) of `horizon` >= 1 steps each -- the clone re-seeded with one draw of the planner's generator (:239), the
 * sampling rule (:42-51), the step (its `done` discarded, :251), get_child with the lowest placeholder left (:207-219), the
 * counts, and partial_value_iteration over the reversed update queue (:89-101) -- then get_plan (graph_based.py:126-135):
 * the root's selection_rule (:53-60) and the chosen chance node's np_random.choice(keys, p=p_minus) (:152-156).
 *   max_next_states must be the handle's (MP_ERR_ARG).  value_max = 1 / (1 - gamma) as the host computes it; accuracy and
 *   sampling_timeout as in the config (a plan holds min(sampling_timeout, 2) entries).  -1 < gamma < 1, accuracy >= 0.
 *   reward_thr_by_count / transition_thr_by_count double [n_counts]: the config's threshold strings evaluated by count 1 ..
 *   n_counts (:69-75, :200-205; the kernel divides the transition threshold by the count, :179).  Counts are LIFETIME counts
 *   of the handle: n_counts must reach mp_gbop_info's max_count plus episodes * horizon (else MP_ERR_ARG); the host extends
 *   its tables by the new counts only.
 *   rng_state uint64 [n,6]: the seed draw of every episode, the tie draws of random_argmax, the double of choice.
 *   action int32 [n] (the model's slot = listing order, -1 without a plan), key int32 [n] (the drawn child: a state, or
 *   -1 - i for "placeholder_i"), plan_len int32 [n] (0, 1 or 2), value_lower / value_upper double [n] (the root's bounds),
 *   env_steps / pops int64 [n] (model steps / queue pops of this call), status int32 [n]: MP_OK,
 *   MP_ERR_GBOP_PLACEHOLDERS (the ValueError of :217-218, after the step was counted), MP_ERR_GBOP_REWARD_THRESHOLD (the
 *   TypeError of :79-82: by then the seed draw, the tie draw, one step and the counts of the first episode are made),
 *   MP_ERR_GBOP_CHOICE_P (numpy's "probabilities do not sum to 1" and its kin), MP_ERR_GBOPD_NO_ACTION (a node no action is
 *   listed for: np.amax([]) in random_argmax, ValueError), MP_ERR_GBOPD_DIVERGED (more than 2^22 pops in one plan),
 *   MP_ERR_ALLOC (queue full) or MP_ERR_ARG (root out of range in a device array).  A planner that reported any of them
 *   stays failed and reports it again.  Changed tables or action sets under a kept graph: as mp_gbopd_plan.
 *   mem as elsewhere (MP_MEM_HOST / MP_MEM_DEVICE / MP_MEM_RNG_DEVICE).  mp_last_kernel_variant reports one of
 *   mp_gbop_form_names: "gbop_{table,dense,sparse}_{lds,global}" (part of no other list); MP_GBOP_LDS_BYTES moves the limit
 *   below which the graph nodes' bounds live in LDS (default 16 KiB, 0: never).
 * mp_gbop_info replaces reading the planner object's sizes; max_count: no count of any planner exceeds it.
 * mp_gbop_export replaces reading planner.nodes: one planner's graph in creation order, arrays of capacity cap >= n_nodes:
 *   state, lower, upper, expanded, count [cap]; per action slot [cap, n_actions]: listed, chance_count, chance_assigned (the
 *   children that stand for a state), chance_backed (that number at the last backup, -1: never backed up), chance_value
 *   [.., 2] (upper, lower); per child SLOT [cap, n_actions, max_next_states] (slot j is placeholder_j until the j-th state
 *   observed takes it; the reference's dict order is slots m .. K-1, 0 .. m-1 for m assigned): child_state (-1 - j for a
 *   placeholder), child_count, child_cumulative_reward, child_mu_ucb, child_mu_lcb; p_plus / p_minus in the dict order of the
 *   backup that wrote them; parent_ptr / parent_idx, visits [n_states], n_observations, root as mp_gbopd_export.
 */
typedef struct mp_gbop mp_gbop;
int mp_gbop_create(mp_ctx *ctx, mp_model *model, int32_t n_planners, int32_t max_next_states, int32_t queue_cap, mp_gbop **out);
int mp_gbop_free(mp_gbop *planners);
int mp_gbop_plan(mp_ctx *ctx, mp_gbop *planners, const int32_t *root_state, int32_t episodes, int32_t horizon,
                 int32_t max_next_states, double gamma, double value_max, double accuracy, int32_t sampling_timeout,
                 int32_t n_counts, const double *reward_thr_by_count, const double *transition_thr_by_count, uint64_t *rng_state,
                 int32_t *action, int32_t *key, int32_t *plan_len, double *value_lower, double *value_upper, int64_t *env_steps,
                 int64_t *pops, int32_t *status, int32_t mem);
int mp_gbop_info(mp_gbop *planners, int32_t *n_planners, int32_t *n_states, int32_t *n_actions, int32_t *max_next_states,
                 int32_t *queue_cap, int64_t *n_edges, int64_t *max_count);
int mp_gbop_export(mp_gbop *planners, int32_t planner, int32_t cap, int32_t *n_nodes, int32_t *state, double *lower, double *upper,
                   uint8_t *expanded, int64_t *count, uint8_t *listed, int32_t *chance_count, int32_t *chance_assigned,
                   int32_t *chance_backed, double *chance_value, int32_t *child_state, int32_t *child_count,
                   double *child_cumulative_reward, double *child_mu_ucb, double *child_mu_lcb, double *p_plus, double *p_minus,
                   int32_t *parent_ptr, int32_t *parent_idx, int64_t *visits, int64_t *n_observations, int32_t *root);
/* The names mp_gbop_plan records for mp_last_kernel_variant, newline separated (host only; part of no other list). */
const char *mp_gbop_form_names(void);

/* ---------------------------------------------------------------- batched evaluation -------- */
/*
 * The env side of Evaluation.step (trainer/evaluation.py:164-190) for n lock-step episodes of ONE deterministic table
 * model, on the device: for every episode i still alive, act = plans[i * plan_stride] (an empty plan, -1, steps label 0
 * and is LOGGED as -1: Evaluation.step raises "The agent did not plan any action" there, evaluation.py:168-170, and so
 * does the caller of this loop),
 *   reward = R[s, act];  done = terminal[s] (or terminal[s'] with done_on_next);  s <- T[s, act];  steps += 1;
 *   returns[i] += reward;  discounted[i] += reward * gpow[steps before];  actions_log[i * log_stride + steps before] = act;
 *   alive[i] = !(done || steps >= max_steps).
 * state / steps int32 [n], alive uint8 [n], returns / discounted double [n] (all in / out); gpow double [max_steps]
 * (gamma ** t as the host computes it); n_alive int32 [1] = episodes still alive after the step.  Episodes that are not
 * alive are left untouched.  The planners' root-state buffers ARE `state` / `steps`: no host round trip per step.
 * mp_greedy_actions: plans[i * plan_stride] = argmax_a Q[state[i], a] (first maximum: ValueIterationAgent.act,
 * value_iteration.py:35) -- the "plan" of a value-iteration agent for the same loop.
 */
int mp_env_step(mp_ctx *ctx, mp_model *model, int32_t n, int32_t *state, int32_t *steps, uint8_t *alive,
                const int32_t *plans, int32_t plan_stride, int32_t max_steps, const double *gpow, double *returns,
                double *discounted, int32_t *actions_log, int32_t log_stride, int32_t *n_alive, int32_t mem);
int mp_greedy_actions(mp_ctx *ctx, int32_t n, int32_t S, int32_t A, const double *Q, const int32_t *state, int32_t *plans,
                      int32_t plan_stride, int32_t mem);
/* mp_env_step for STOCHASTIC / sparse models: the next state is sampled from the episode's own env generator record
 * (env_rng uint64 [n, 6], numpy PCG64, advanced in place) exactly as FiniteMDPEnv.step does -- one Generator.random()
 * double, inverse CDF over the row.  The planner reads the same records (mp_uct_plan_stochastic's env_rng_state): every
 * plan's clones start from the env generator as it is at that step. */
int mp_env_step_stochastic(mp_ctx *ctx, mp_model *model, int32_t n, int32_t *state, int32_t *steps, uint8_t *alive,
                           const int32_t *plans, int32_t plan_stride, int32_t max_steps, const double *gpow, double *returns,
                           double *discounted, int32_t *actions_log, int32_t log_stride, int32_t *n_alive, uint64_t *env_rng,
                           int32_t mem);

/* ---------------------------------------------------------------- result exchange ------------ */
/*
 * The one exchange of the sharded planning path (per-root {plan, value, env_steps} to every rank; the
 * reference has no counterpart -- one process per experiment, scripts/experiments.py:102-106).  Both calls work on DEVICE
 * buffers only and only enqueue (on `stream`, a hipStream_t, or on the ctx stream when NULL): the caller runs ONE
 * all_gather_into_tensor (RCCL) on `packed` between them, no host hop.
 *   mp_pack_rows:   n_arrays (<= 8) per-root arrays src[k] with row widths width[k] bytes (multiples of 4) of this
 *                   rank's n_local roots -> packed uint8 [per][row_bytes], row_bytes = sum(width); rows n_local..per-1
 *                   (the padding that makes every rank's block the same size) are zero-filled.
 *   mp_unpack_rows: gathered uint8 [world][per][row_bytes] -> dst[k] [n_total][width[k]]; global row i comes from
 *                   rank r's block where [lo_r, hi_r) is the balanced contiguous split of n_total over world ranks
 *                   (the first n_total % world ranks hold one row more), i.e. rl_agents_amd.distributed.shard_bounds.
 * src / dst / width are HOST arrays of device pointers / ints.
 */
int mp_pack_rows(mp_ctx *ctx, void *stream, int32_t n_local, int32_t per, int32_t n_arrays, const void *const *src,
                 const int32_t *width, void *packed);
int mp_unpack_rows(mp_ctx *ctx, void *stream, int32_t n_total, int32_t world, int32_t per, int32_t n_arrays,
                   const void *packed, const int32_t *width, void *const *dst);

/*
 * The collective itself, for a consumer that has no torch.distributed (mp_comm_init / mp_gather_results): RCCL,
 * resolved at run time (dlopen of librccl.so.1 -- the copy already in the process if there is one, e.g. PyTorch's -- so the
 * library has no link-time dependency on it).  One communicator per ctx, one rank per GPU.
 *   mp_comm_unique_id: rank 0 creates the 128-byte id (ncclGetUniqueId); the caller hands it to the other ranks out of band
 *                      (a file, a socket, MPI: whatever launched the ranks).
 *   mp_comm_init:      ncclCommInitRank on the ctx's device; collective over all `world` ranks.
 *   mp_gather_results: ncclAllGather of this rank's packed block (per * row_bytes bytes, from mp_pack_rows) into
 *                      gathered [world][per][row_bytes] on `stream` (NULL: the ctx stream); device buffers, only enqueues.
 *                      mp_unpack_rows then spreads the rows into the per-root arrays.
 *   mp_comm_destroy:   ncclCommDestroy (also done by mp_ctx_destroy).
 * rl_agents_amd.distributed.ShardedDevicePlan uses torch.distributed's process group instead (the host side of this
 * package is PyTorch); tests/test_gpu_distributed.py checks that both deliver the same bytes.
 */
#define MP_COMM_UID_BYTES 128
int mp_comm_unique_id(void *uid);
int mp_comm_init(mp_ctx *ctx, int32_t rank, int32_t world, const void *uid);
int mp_gather_results(mp_ctx *ctx, void *stream, int32_t per, int32_t row_bytes, const void *packed, void *gathered);
int mp_comm_destroy(mp_ctx *ctx);

/* ---------------------------------------------------------------- helpers ------------------- */
/* OLOP.allocation (tree_search/olop.py:50-62) with OLOP.horizon (:42-44); host arithmetic. */
int mp_olop_allocation(int32_t budget, double gamma, int32_t *episodes, int32_t *horizon);
/* The kernel form mp_uct_plan* chooses for a call of this description, on the host alone (no device, no ctx: tests pin the choice
 * without a GPU).  The MP_UCT_* knobs are read from the environment as the plan reads them.
 *   call[14]: n_roots, episodes, horizon, |A|, the model's S, NB and Sb (batch models: MDPs, states per MDP), compact transitions
 *             (0 / 1), compact reward index (0 / 1), distinct rewards, CartPole (0 / 1), policy (0 none, 1 per-state, 2 listed),
 *             the layout of the kept tree the plan continues (-1: fresh trees), compute units.
 *   out[7]:   tree layout, lanes, waves, rep_shift (the kernel arguments), roots and threads per workgroup, dynamic LDS bytes.
 *   *name:    the form, as mp_last_kernel_variant names it.
 * A call the plan refuses for its shape gets the plan's MP_ERR_ARG. */
int mp_uct_choose_form(const int64_t *call, int64_t *out, const char **name);
/* The same for a call of mp_saopd_plan (host only); the MP_SAOPD_* knobs are read as the plan reads them, the planners' mapping is
 * the one mp_saopd_create would give them now (|A| and MP_SAOPD_MODEL).
 *   call[10]:  n_planners, the model's S and |A|, budget, what the planners hold per planner: node rows in use (mp_saopd_info; 0:
 *              fresh), rows and queue entries allocated (0: none yet, or not known: the form depends on neither unless
 *              MP_SAOPD_QUEUE is smaller than the queue they have), costs to sort by (0 / 1: an earlier plan of these planners, or
 *              of another batch on the model), device arrays (0 / 1), compute units.
 *   out[20]:   wave mapping (0 / 1), K, node rows after the plan, rows and queue entries allocated for it, chunk-pool ints, the
 *              kernel arguments tab_plain, tab_lds, lds_rows, lds_qcap, scap (first launch / global-memory queue), par_backup,
 *              csr_old, prune_rows, sticky, whether the dispatch order is sorted, the dynamic LDS bytes of the first launch and of
 *              the fallback, the byte limit of a growing queue.
 *   *name:     the first launch, as mp_last_kernel_variant names it, "_ordered" included, never "_retry".
 *   *fallback: the form a call whose backup queue fills up runs again on (recorded with "_retry").
 * A call the plan refuses for its sizes gets the plan's MP_ERR_ARG. */
int mp_saopd_choose_form(const int64_t *call, int64_t *out, const char **name, const char **fallback);
/* Timing of the last kernel batch enqueued by a plan / solve call, from HIP events recorded on
 * the ctx stream around the kernel launches only (no copies).  Synchronises the stream. */
int mp_last_kernel_ms(mp_ctx *ctx, double *ms, int32_t *n_launches);
/* Name of the kernel form the last plan call of any planner, or the last mp_vi_solve_batch, launched on this ctx: every selector
 * that changes which device code runs, after all overrides and fallbacks.
 *   UCT           "uct_global", "uct_ldsr" (model resident in LDS), "uct_quad" (four lanes per root), "uct_lone" (one root per
 *                 workgroup), "uct_lone_mw" (2 / 4 / 8 roots per workgroup, a wavefront each, around one copy of the
 *                 transitions), "uct_row_shared" / "uct_row_each" / "uct_lone_each" (four roots per wavefront on DPP rows, trees
 *                 in LDS: a shared model / one MDP per root; a wavefront per root), "uct_policy", "uct_cartpole",
 *                 "uct_global_spill"
 *   batched VI    "vi_batch_reg<own,block>", "vi_batch_cluster2|4|8" (K workgroups per MDP), "vi_batch_wg_stream|lds|global"
 *   OLOP, BRUE    "olop_global", "brue_global" (a tree per root, kept for the export), "..._slots" (slots shared by the waves);
 *                 one MDP per root (mp_olop_plan_models / mp_brue_plan_models): "olop_each_lds" / "olop_each_global",
 *                 "brue_each_lds" / "brue_each_global", then "_slots"
 *   GBOP-D        "gbopd_wave_lds", "gbopd_wave_global"
 *   Sparse        "ss_wave_lds", "ss_wave_global" (the frames of the recursion in LDS / in a global workspace); one MDP per root
 *   Sampling      (mp_ss_plan_models): "ss_each_lds" / "ss_each_global"
 *   MDP-GapE      "gape_global", then "_slots"; one MDP per root (mp_gape_plan_models): "gape_each_lds" / "gape_each_global", then
 *                 "_slots" (listed by mp_gape_form_names / mp_gape_each_form_names, not by mp_kernel_form_names); with transition
 *                 bounds "gape_stoch_{table,dense,sparse}", one MDP per root "gape_stoch_each_lds" / "gape_stoch_each_global",
 *                 then "_slots" (mp_gape_stoch_form_names / mp_gape_stoch_each_form_names)
 *   OPD           "opd_any" (more than 64 actions); "opd_lds" / "opd_ldsx" (bounds in LDS / the parent map in HBM), then "_gen"
 *                 (the main loop for arbitrary bounds), then "_chain" (the closing pass on the node array);
 *                 "opd_wide_sib" / "opd_wide_cls" (bounds in HBM, sibling / residue-class layout), then "_small" (at most two
 *                 slots per lane in a re-scan), then "_gen"
 *   robust OPD    "ropd_any"; "ropd_lds" / "ropd_ldsx", then "_m2" / "_m4" (batched loads for up to two / four models) or "_gen",
 *                 then "_chain"; "ropd_wide_sib" / "ropd_wide_cls", then "_gen"
 *   state-aware   "saopd_lane" (a planner per lane), "saopd_wave" (per wavefront), "saopd_wave_dict" (dictionaries in LDS),
 *                 "saopd_wave_lds" (the arena in LDS too): the kernel of the call's LAST launch; then "_ordered" (the dispatch
 *                 order was sorted), then "_retry" (the call rolled back and ran again)
 *   stochastic    "uct_stoch_r{0,2,4,1}_p{16,32}_a{any,2..8}", then "_policy": step records (0 rows and thresholds, 2 / 4 fused
 *   UCT           records of that many successors, 1 compact 16-byte records), bits of a path entry, the unrolled |A|
 * The host picks by model, batch size and the MP_* test hooks; reports and tests name what ran.  Results do not depend on the form. */
const char *mp_last_kernel_variant(mp_ctx *ctx);
/* 1 if the last mp_uct_plan / mp_uct_plan_models / mp_uct_plan_policy call on ctx launched its form with the rollout's action
 * table in LDS ("uct_ldsr", |A| <= 6, a state-independent policy, 4 096 bytes of LDS to spare, MP_UCT_ACTION_TABLE not 0), 0 if
 * it launched the form with the exact compares in every rollout step, or if no such call was made.  The form's name is the same
 * either way, and so are the results: tests that force an arm assert it with this. */
int mp_uct_last_action_table(mp_ctx *ctx);
/* Every name mp_last_kernel_variant can return, one per line, built by the functions that name the launches (host only, no
 * device): a test table that is to cover every form is compared with this list.  (Sparse Sampling's two names are listed by
 * its own mp_ss_form_names, single-model value iteration's by mp_vi_form_names, the one-MDP-per-root forms of OLOP and BRUE by
 * mp_each_form_names, those of Sparse Sampling by mp_ss_each_form_names.) */
const char *mp_kernel_form_names(void);
/* Hardware self-test (no reference counterpart): LDS atomics of ONE wavefront instruction that hit the same address apply
 * in LANE ORDER on this device -- the state-aware OPD kernel's grouped backup relies on it (one ds_min_rtn_f64 of the group
 * leaders hands every leader the running minimum the reference's turn-by-turn loop would have read).  Runs `waves` wave
 * instructions with random lane masks / addresses / values; *violations = returned values that are not the lane-order
 * prefix minimum + wrong final cells (0 on a conforming device). */
int mp_selftest_lds_atomic_order(mp_ctx *ctx, int32_t waves, int64_t *violations);

#ifdef __cplusplus
}
#endif
#endif /* MI355PLAN_H */
