// uct.hip -- MCTS/UCT planning (tree_search/mcts.py) for thousands of independent roots.
//
// Mapping: ONE ROOT PER LANE.  A root's plan() is inherently sequential (every episode reads
// the tree the previous one updated; every env step depends on the previous state), so the
// parallel axis is roots.  A cloned environment (reference: safe_deepcopy_env,
// common/factory.py:119-134) is an (int32 state, int32 steps) register pair.  A batch takes as
// long as its slowest lane's dependency chain, so the kernel is built to shorten that chain:
//
//   model   default: one 16-byte record {next, flags, reward} per (s,a), a single dwordx4 gather per
//           env step (any S).
//           ENV_TABLE_LDSR (round 4, the default wherever the model fits): the WHOLE model lives in LDS -- uint16
//           transitions {bit15 = terminal[next], next state}, a uint8 index per (s,a) into the table of the model's
//           distinct rewards (<= 256 of them) and that
//           table -- 3 B per (s,a): the headline's S*A = 50 000 takes 150 of the CU's 160 KB.  An env step then makes
//           no global-memory request at all; the path stack moves from LDS to registers (depths 1..5) with a global
//           spill beyond.  One workgroup of up to 16 waves per CU shares the tables.
//           ENV_CARTPOLE: closed-form dynamics, state in registers.
//   rng     numpy PCG64 stepped per lane (pcg64.hpp, 128-bit multiply on 32-bit limbs); the draw for
//           step h+1 is computed on a second generator copy while step h's lookup is in flight and
//           kept only if the rollout continues, so the stream stays bit-identical to the reference's.
//           Rollout actions come from integer thresholds ceil(cdf * 2^53) <= (next64 >> 11).
//   tables  gamma**h, the thresholds, 1/n and temperature*|A|*prior[a]/n for every visit count n of a
//           fresh tree are computed on the host with the reference's own operations (libm pow, IEEE
//           divide) and read from LDS; larger counts (kept trees) use the device's IEEE division.
//   tree    Node[n_roots][cap] root-major 16-byte records {value f64, count i32, first_child i32}
//           in HBM; the A children of a node are contiguous.  cap = 1 + episodes*A (+ the kept tree).
//           The root and its children (ids 0..A) live in registers for the whole plan, and the path
//           nodes of depths 2..5 keep the statistics their selection read until the backup: the
//           saturated kernel is bound by L2/HBM requests, and these remove a third of them.  A node below them is written ONCE per
//           episode: the backup stores value and count in one 12-byte store, and the leaf whole (16 bytes) with the first_child
//           its expansion assigned -- no store of its own for that.  The forms that gather the model from global memory write
//           the zero nodes of a wave's expansions lane-contiguously (the group-interleaved layout: one run per group and wave)
//           instead of |A| strided nodes per lane (uct_kernel, TREE STORES; profiles/uct_tree_stores.md).  The children of a node
//           that was visited once are all zero nodes: they are not loaded, and a fresh tree does not store them before they are
//           entered (uct_kernel, VIRGIN GROUPS; uct_virgin.hpp; profiles/uct_virgin_groups.md).  A fresh tree stores only the
//           children an episode picked and marks them in the upper bits of the parent's first_child: the others are neither
//           stored nor loaded (uct_kernel, VISITED MASK; profiles/uct_visited_mask.md).  The plan's read-out takes the root and
//           its children from the registers that hold them and costs one round trip per level below (uct_kernel, READ-OUT FROM
//           REGISTERS; profiles/uct_step_fixed_costs.md).
//   path    per-lane stack of visited node ids in LDS ([depth][lane], conflict-free): the backup
//           walks known addresses, not parent pointers.
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include <type_traits>

#include "common.hpp"
#include "libm_sincos.hpp"
#include "pcg64.hpp"
#include "uct_action_table.hpp"
#include "uct_balance.hpp"
#include "uct_host.hpp"
#include "uct_virgin.hpp"
#include "wave.hpp"

namespace mp {

struct alignas(16) UctNode {
    double value;
    int32_t count;
    int32_t first_child; // -1 = not expanded
};
static_assert(sizeof(UctNode) == 16, "UctNode must be one dwordx4");

// One root's tree inside the batch buffer.  LAY selects the layout (A/B: profiles/r02_uct_tree_layout.md):
//   0 root-major       Node[n_roots][cap]: a root's nodes contiguous -- the |A| children of a node share one or two
//                      cache lines, but neighbouring lanes are a whole tree apart: nothing a wave does coalesces.
//                      Generic |A| and CartPole.
//   2 group-interleaved Node[n_roots / 64][groups][64][|A|]: node ids come in groups of |A| siblings (1 + g|A| .. ;
//                      the root fills the last slot of group 0); a lane's sibling group stays contiguous (one or two
//                      lines per scored level, as root-major) AND the same group of the 64 lanes is contiguous
//                      (expansions write 64 x |A| x 16 B = one run).  Needs |A| at compile time.
// Hot sites address a child through its sibling group (child / handle: one add and a shift); operator[] maps any id.
template <int LAY, int AT>
struct TreeRef {
    UctNode *base;
    int A; // runtime |A| (generic ids only)
    // node fc + a where fc is the first child of some node (fc = 1 mod |A|)
    __device__ __forceinline__ int handle(int fc, int a) const { return LAY == 2 ? ((fc - 1 + AT) << 6) + a : fc + a; }
    __device__ __forceinline__ int root_handle() const { return LAY == 2 ? AT - 1 : 0; }
    __device__ __forceinline__ UctNode &at(int h) const { return base[(unsigned)h]; }
    __device__ __forceinline__ UctNode &child(int fc, int a) const { return at(handle(fc, a)); }
    // sibling a of a group whose first node is *first (= &child(fc, 0)): one address computation per group, the siblings
    // at constant offsets (the compiler cannot derive that from 32-bit handles: it re-materialises a 64-bit address each)
    __device__ __forceinline__ static UctNode &sibling(UctNode *first, int a) { return first[a]; }
    __device__ __forceinline__ UctNode &operator[](int n) const
    {
        if (LAY != 2) return base[(unsigned)n];
        const int x = n + A - 1, q = x / A;          // group q (root: group 0, last slot), slot x - q|A|
        return base[(unsigned)(q * A * 64 + (x - q * A))];
    }
};
template <int LAY, int AT>
__device__ __forceinline__ TreeRef<LAY, AT> tree_of(UctNode *trees, int r, int cap, int A)
{
    TreeRef<LAY, AT> t;
    t.A = A;
    if (LAY == 2) t.base = trees + ((long)(r >> 6) * (cap + A) * 64 + (long)(r & 63) * A);
    else t.base = trees + (long)r * cap;
    return t;
}
// nodes to allocate per root for a layout
static inline size_t tree_stride_alloc(int lay, long cap, int A) { return (size_t)(lay == 2 ? cap + A : cap); }

struct UctArgs {
    int n_roots, S, A, episodes, horizon, cap;
    int table_n; // counts with entries in the quotient tables of `tab` (TE below): min(episodes, what 16 KB of LDS hold)
    int tree_il; // tree layout (TreeRef): 0 root-major, 2 group-interleaved
    int done_on_next, max_steps, max_plan_len;
    int lanes; // roots per wavefront (64 = dense; fewer spreads a small batch over more SIMDs)
    int rep_shift; // CartPole: a root is replicated over 2^rep_shift lanes (see the launch code: wavefronts of few ACTIVE lanes run slow)
    int waves; // wavefronts per workgroup
    int tree_stores; // 1: a full wave writes its expansions' zero nodes lane-contiguously and the backup stores the leaf whole;
                     // 2 (MP_UCT_TREE_STORES=virgin): as 1, and virgin groups are not loaded and, in fresh trees, not stored (VIRGIN
                     // GROUPS below); 3 (the default; the host passes it for fresh trees of a form of uct_mask_form only, else 2): as
                     // 2, and only the children an episode picked are stored or loaded (VISITED MASK below);
                     // 0 (MP_UCT_TREE_STORES=lane, an A/B knob): every store per lane, first_child of an expanded node on its own
    int balance; // host side only: 1 launches the BAL instantiation of the one-lane LDS-resident form (WAVE BALANCE in uct_kernel) with
                 // 64 more bytes of LDS; 0: MP_UCT_BALANCE=0, any other form, or a model that leaves no room for them
    int action_table; // host side only: 1 launches the ATAB instantiation of that form (ACTION TABLE in uct_kernel) with kUctActBytes
                      // more of LDS; 0: MP_UCT_ACTION_TABLE=0, any other form or policy, or a model that leaves no room for them
    int Sb;    // batch models: states per MDP (root r plans on MDP root_state[r] / Sb); = S for any other model
#ifdef MP_WAVE_STAMPS
    unsigned long long *wave_stamps; // diagnostic build: [waves of the launch][kWaveStampWords], or nullptr (WAVE STAMPS in uct_kernel)
#endif
    const Rec *rec;
    const uint16_t *t16; // compact transitions (LDS variants), [S*A]
    const uint8_t *r8;   // LDS-resident variant: index of reward[s, a] in rdict, [S*A]
    const double *rdict; //                       the model's distinct reward values, [n_rdict] (<= 256)
    int n_rdict;
    const uint32_t *jump; // four-lanes-per-root variant: limbs of A^n and G_n, n = 0..H (PCG64 jump-ahead), [H + 1][8]
    int32_t *path_spill; // LDS-resident variant: path handles of depths the registers do not hold, [H + 1][spill_stride]
    long spill_stride;
    const int32_t *root_state, *root_steps;
    const double *root_x; // CartPole roots: [n_roots][4] = x, x_dot, theta, theta_dot
    mp_cartpole_params cp;
    int cp_sincos;       // how CartPole's sin / cos are evaluated (libm_sincos.hpp: 0 device, 1 / 2 the host libm's forms)
    int cp_fastdiv;      // 1: the parameters qualify for div_by_const (host check in the launch code)
    double cp_inv_tm;    // RN(1 / total_mass)
    const double *tab; // gpow[H+1] | thr[A] (uint64 bits) | tp[A] | rcp[TE+1] | tpdiv[A][TE+2]
    uint64_t thr_arg[8]; // the same thresholds by value (|A| <= 8), SHIFTED UP by 11 bits (compared with the raw 64-bit draw; 2^53 -> ~0): kernel arguments live in SGPRs
    int thr_valid;       // how many of the first |A| - 1 thresholds are below 2^53 (the others can never be reached)
    const uint8_t *act_tab; // action_table: the kUctActBytes entries of uct_action_table_fill for thr_arg / thr_valid, else nullptr
    // per-state policies (mp_policy): nullptr / 0 for the state-independent ones
    const double *pol_prior; // [S][pol_stride]
    const uint64_t *pol_thr; // [S][pol_stride]
    const uint4 *pol_frec;   // [S*A][1 + ceil((A-1)/4)]
    const uint4 *pol_frec_roll; // the same records laid out by ROLLOUT slot (= pol_frec unless the rollout policy lists the actions in another order)
    int pol_stride;
    int pol_shift;           // fused thresholds = min(thr >> pol_shift, pol_sat); 21 = the top 32 of 53 bits
    uint32_t pol_sat;        // 2^32 - 1, or 1023 for the packed 16-byte records
    int pol_packed;          // 1: 16-byte records {next:20 | th0:10, flags:2 | th1:10 | th2:10 | th3:10, reward f64}
    double TA;               // temperature * |A|  (mcts.py:286, left to right)
    double temperature;      // listed policies: the factor is temperature * len(children) of the node being scored
    uint64_t *rng;
    UctNode *tree;
    const int32_t *n_nodes_in; // kept (re-rooted) tree sizes, nullptr = every root starts fresh
    int32_t *n_nodes_out;
    int32_t *plans, *plan_len;
    double *root_value, *root_child_value;
    int64_t *root_child_count, *env_steps;
};


// a / b for a CONSTANT b whose correctly rounded reciprocal y = RN(1 / b) the host supplies, as five multiply-adds: q0 = RN(a y) is
// within two ulps of a / b, q1 = RN(q0 + r0 y) with the exact residual r0 = a - b q0 lies within 2^-100 of a / b before its rounding,
// hence is a faithful quotient, and q2 = RN(q1 + r1 y) is then the CORRECTLY ROUNDED a / b (Markstein 1990; Muller et al., Handbook
// of Floating-Point Arithmetic, ch. 4.7: holds unless b's significand is all ones) -- the same bits as the IEEE division, which
// the hardware does in thirteen instructions (v_div_scale x 2, v_rcp, four refinements, v_div_fmas, v_div_fixup).  Exact while
// the residuals are: a = 0, or 2^-960 <= |a| <= 2^1000 (the CartPole rollout proves that range from a bound on the pole's
// velocity it tracks; see there); b normal.
__device__ __forceinline__ double div_by_const(double a, double b, double y)
{
    const double q0 = a * y;
    const double r0 = __fma_rn(-q0, b, a);
    const double q1 = __fma_rn(r0, y, q0);
    const double r1 = __fma_rn(-q1, b, a);
    return __fma_rn(r1, y, q1);
}
// lane I of every DPP row (16 lanes), to the row's lanes (row_newbcast:I)
template <int I>
__device__ __forceinline__ uint32_t row_bcast(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x150 + I, 0xf, 0xf, false);
}
// lane Q of every quad, to the quad's four lanes (DPP quad_perm Q,Q,Q,Q)
template <int Q>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, Q * 0x55, 0xf, 0xf, true);
}

// rl_agents_amd/envs/cartpole.py step(), operation for operation in IEEE double (no contraction).
// sin / cos of the pole angle: the HOST libm's algorithm restated (libm_sincos.hpp; `sincos_mode` = the form that
// reproduces this host's sin / cos, found at model-load time) -- bit-exact plans by construction since round 5; mode 0 = the
// device math library (last bit may differ from glibc's: the tolerance of rounds 1-4).
__device__ __forceinline__ bool cartpole_step(const mp_cartpole_params &c, double (&x4)[4], int act, int sincos_mode, const double *sctab)
{
    const double total_mass = c.masspole + c.masscart, polemass_length = c.masspole * c.length;
    double x = x4[0], x_dot = x4[1], theta = x4[2], theta_dot = x4[3];
    const double force = act == 1 ? c.force_mag : -c.force_mag;
    double sintheta, costheta;
    libm_sincos(sincos_mode, theta, &sintheta, &costheta, sctab);
    const double temp = (force + polemass_length * (theta_dot * theta_dot) * sintheta) / total_mass;
    const double thetaacc = (c.gravity * sintheta - costheta * temp) /
                            (c.length * (4.0 / 3.0 - c.masspole * (costheta * costheta) / total_mass));
    const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
    x = x + c.tau * x_dot;
    x_dot = x_dot + c.tau * xacc;
    theta = theta + c.tau * theta_dot;
    theta_dot = theta_dot + c.tau * thetaacc;
    x4[0] = x; x4[1] = x_dot; x4[2] = theta; x4[3] = theta_dot;
    return x < -c.x_threshold || x > c.x_threshold || theta < -c.theta_threshold || theta > c.theta_threshold;
}

// a progress word of the wave balance (uct_balance.hpp), read and written as a relaxed atomic of the workgroup: a plain LDS read or
// write that the compiler neither keeps in a register nor moves out of the episode loop -- other waves write the words
__device__ __forceinline__ uint32_t bal_load(const uint32_t *w) { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void bal_store(uint32_t *w, uint32_t v) { __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the SIMD of its CU that the wave runs on (HW_ID bits 5:4); a wave stays where it was placed
__device__ __forceinline__ uint32_t simd_id()
{
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 4, 2)" : "=s"(v));
    return v;
}
#ifdef MP_WAVE_STAMPS
constexpr int kWaveStampWords = 8;   // 64-bit words per wave: entry, staged, last episode done, exit, HW_ID | XCC_ID << 32 (three unused)
#endif

enum { ENV_TABLE = 0, ENV_CARTPOLE = 2, ENV_TABLE_LDSR = 3, ENV_TABLE_SPILL = 4 };
// ENV_TABLE_SPILL: ENV_TABLE with the path stack in registers + a global spill array instead of LDS -- for horizons whose
// [H + 1][64] stack would not fit (the reference has no horizon limit: tree_search/mcts.py:116-118)

// AT > 0: |A| known at compile time (children scored from registers in one pass);
// AT == 0: any |A| (three passes over the children).  ENV: where an env step comes from.
#ifndef MP_UCT_MIN_WAVES
#define MP_UCT_MIN_WAVES 1
#endif
#ifndef MP_PCG_WORDS
#define MP_PCG_WORDS 1
#endif
// -DMP_UCT_MASK_LOADS=0 builds the visited-mask form (VM) with the whole group loaded wherever any child of it was stored, instead
// of one predicated load per stored child: the dropped sibling stores alone, for A/B runs (profiles/uct_visited_mask.md).
#ifndef MP_UCT_MASK_LOADS
#define MP_UCT_MASK_LOADS 1
#endif
// -DMP_UCT_READOUT_REGS=0 builds uct_kernel's plan read-out with every value loaded back from the tree, for A/B runs
// (profiles/uct_step_fixed_costs.md).
#ifndef MP_UCT_READOUT_REGS
#define MP_UCT_READOUT_REGS 1
#endif
// The instantiations of uct_kernel whose one-lane table rollout runs on Pcg64W: every table form (CartPole draws in its own
// loops, the four-lane form jumps instead of stepping).
constexpr bool uct_pcg_words_form(int AT, int ENV, bool SP, bool MK, int IL, bool QD)
{
    return ENV != ENV_CARTPOLE && !QD;
}
// THE LEAN TRIP (profiles/uct_lean_trip.md): vector instructions of that rollout's trip of two env steps which the result does
// not need, each part behind a macro of its own (default on; =0 builds the part as it was, for A/B runs):
//   MP_UCT_TERM_TABLE   the terminal rule is in the staged table, not in the kernel (uct_term_table.hpp): one compare of the
//                       record's bit 15 per step, in the descent as well; no `cur_term`, no select by done_on_next.  The
//                       one-lane LDS-resident form only (the four-lane form, uct_lone_kernel and uct_row_kernel stage the
//                       next-state table and keep the rule); the host hands the form the table of the model's rule
//   MP_UCT_LEAN_INDEX   the record word is a 32-bit value from its load on: no zero-extension of the 15-bit next state
//   MP_UCT_LEAN_COUNT   one add to the step counter per trip, compared with the last step in both steps
//   MP_PCG_NO_C1        pcg64.hpp: no compare for the column-1 carry of Pcg64W
#ifndef MP_UCT_TERM_TABLE
#define MP_UCT_TERM_TABLE 1
#endif
#ifndef MP_UCT_LEAN_INDEX
#define MP_UCT_LEAN_INDEX 1
#endif
#ifndef MP_UCT_LEAN_COUNT
#define MP_UCT_LEAN_COUNT 1
#endif
constexpr bool uct_term_table_form(int ENV, bool QD)
{
    return MP_UCT_TERM_TABLE != 0 && ENV == ENV_TABLE_LDSR && !QD;
}
// SP: the prior and the rollout distribution are rows of per-state tables (mcts_with_prior.py:47-62).  The env is
// deterministic, so the state a node is reached in is a function of its action sequence and the prior stored in a
// child at expansion (mcts.py:237-246) is prior[state of the parent][action]: it is looked up with the state the
// descent is in, not stored.  Rollouts read one fused 32-byte (|A| <= 5) or 48-byte record per step -- the (s,a)
// record followed by the sampling thresholds of the state it leads to -- so the per-step dependency chain stays one
// gather long.  The fused thresholds are the top 32 of the 53 bits: they decide the draw unless one of them equals
// the draw's top 32 bits (probability ~|A| * 2^-32 per step), in which case the exact 53-bit row is fetched.
// MK (with SP): the prior policy lists only a subset of the actions per state (restricted action sets, mcts.py:59-97).  An
// expansion still appends |A| node slots so that ids stay lock-step across lanes, but the slots of unlisted actions are
// PHANTOMS (count = -1): never scored, never visited, dropped by the tree export.  The listed-action masks of the state
// reached / acted from ride in bits 8-15 / 16-23 of the fused records' flags word, so the descent always knows the mask
// of the state it is in without another gather; len(children) in the exploration term is the mask's population count.
// QD (with ENV_TABLE_LDSR; round 5): FOUR LANES PER ROOT, for batches too small to fill the chip (SURVEY 8(d)'s own sizes: 4096
// roots, one root).  A lone wave per SIMD runs at the latency of its dependency chain, and in a rollout step that chain is
// numpy's PCG64 (next64 compiles to 35 vector instructions in isolation, a step of the one-lane loop to 56) + the model
// lookup.  With state-independent policies the ACTION
// SEQUENCE of a rollout does not depend on the states it visits: the four lanes of a root draw the rollout's H actions four
// at a time -- lane j holds the generator j + 1 steps ahead and jumps by four per round (state <- A^4 state + inc G_4: one
// 128-bit multiply, as a single step) -- and the root's first lane (its OWNER: tree phases are its alone) walks the model in
// LDS through each round's four actions while the next round's draws are computed beside it: per step one LDS lookup on the
// state chain and no generator arithmetic.  The walk consumes n draws; the generator then jumps by exactly n (limbs of A^n,
// G_n from a table), so the stream stays the reference's.  Same trees, plans and generator states as every other variant.
// BAL (the one-lane LDS-resident form): WAVE BALANCE below -- a template argument, not a kernel argument, because the form has no
// scalar register left for a flag that lives over the whole plan (a run-time flag spilled in five of its seven instantiations).
// VM (the forms of uct_mask_form, fresh trees): VISITED MASK below -- a template argument for the same reason.
// ATAB (the forms of uct_action_table_form): ACTION TABLE below -- a template argument for the same reason.
template <int AT, int ENV, bool SP = false, bool MK = false, int IL = 0, bool QD = false, bool BAL = false, bool VM = false,
          bool ATAB = false>
// Per-state-policy kernels with |A| <= 5 are held to the registers of 4 waves per SIMD (they would take 134-140 VGPRs = 3
// waves; TA 52 %, VALU 45 %, L1 28 % busy: latency-bound -- 2.14 -> 1.91 ms at 262 144 roots with the fourth wave).
__global__ __launch_bounds__(ENV == ENV_TABLE_LDSR ? 1024 : (ENV == ENV_CARTPOLE ? 256 : 64),
                             ENV == ENV_TABLE_LDSR ? 1 : (SP && AT > 0 && AT <= 5 && MP_UCT_MIN_WAVES < 4 ? 4 : MP_UCT_MIN_WAVES))
void uct_kernel(UctArgs p)
{
    static_assert(!SP || (AT > 0 && ENV == ENV_TABLE), "per-state policies: table env, |A| known at compile time");
    static_assert(!MK || SP, "listed policies are per-state policies");
    constexpr int NTH = AT > 1 ? AT - 1 : 1; // thresholds that can be reached (the last one is 2^53: never)
    constexpr int NQ = (NTH + 1) / 2;        // 16-byte chunks of a row of exact (uint64) thresholds
    constexpr int NQ32 = (NTH + 3) / 4;      // 16-byte chunks of the fused record's 32-bit thresholds
    constexpr bool LDSR = ENV == ENV_TABLE_LDSR;             // transitions AND rewards in LDS (the reward one step behind the
                                                             // state chain), path stack in registers
    static_assert(!LDSR || (AT > 0 && !SP), "the LDS-resident variant: |A| at compile time, state-independent policies");
    static_assert(!QD || LDSR, "four lanes per root: the LDS-resident model");
    constexpr bool PREG = LDSR || ENV == ENV_TABLE_SPILL;    // path stack in registers + global spill, not in LDS
    constexpr bool CART = ENV == ENV_CARTPOLE;
    // RAWU: the rollout compares the generator's raw 64-bit output with thresholds shifted up by 11 bits (thr <= out >> 11
    // <=> thr << 11 <= out) instead of shifting every draw down to its 53 random bits
    constexpr bool RAWU = AT > 0 && !SP;
    constexpr int USH = RAWU ? 0 : 11;
    static_assert(!BAL || (LDSR && !QD), "the wave balance: the one-lane LDS-resident form");
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    // BAL: the sixteen progress words come FIRST, at an address known at compile time, and everything else moves up by their 64
    // bytes (the launch adds them to the form's LDS size): behind the model their address would be one more value to keep
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_bal[];   // (the same bytes as lds_raw: every dynamic array starts there)
    // ATAB: the action table directly behind them, at a compile-time address as well, and everything else moves up by it too
    static_assert(!ATAB || uct_action_table_form(AT, ENV, SP, MK, IL, QD), "the action table: the forms of uct_action_table_form");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_bytes[];  // (the same bytes again)
    const uint8_t *lds_act = lds_bytes + (BAL ? kUctBalBytes : 0);       // [kUctActBytes]
    double *lds_d = lds_raw + ((BAL ? kUctBalBytes : 0) + (ATAB ? kUctActBytes : 0)) / sizeof(double);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int A = AT > 0 ? AT : p.A, H = p.horizon, E = p.episodes;
    const int nthreads = p.waves * 64;
    double *gpow = lds_d;                   // [H + 1]  gamma ** h
    // rollout policy as integer thresholds: u = k * 2^-53 with k = next64 >> 11, and
    // searchsorted(cdf, u, 'right') = #{a : cdf[a] <= u} = #{a : ceil(cdf[a] * 2^53) <= k}
    const uint64_t *thr = reinterpret_cast<const uint64_t *>(gpow + (H + 1)); // [A]
    double *tp = gpow + (H + 1) + A;        // [A]      temperature * |A| * prior[a]
    const int TE = p.table_n;               // counts the quotient tables cover
    double *rcp = tp + A;                   // [TE + 1]  1.0 / n
    double *tpdiv = rcp + (TE + 1);         // [A][TE+2] temperature * |A| * prior[a] / n
    const int ntab = (H + 1) + 2 * A + (TE + 1) + A * (TE + 2);
    // visit counts beyond the tables (trees kept across plans, step_strategy "subtree"; plans of more episodes than the
    // tables hold) take the IEEE division itself -- the same correctly rounded quotient the host put in the tables
    auto explore = [&](int a, int cnt1) { return cnt1 <= TE + 1 ? tpdiv[a * (TE + 2) + cnt1] : tp[a] / (double)cnt1; };
    auto inv = [&](int c) { return c <= TE ? rcp[c] : 1.0 / (double)c; };
    // The same quotients for the register-held tree phase (AT > 0): the table entry at a CLAMPED index, read unconditionally --
    // no test, branch or wait of its own per child, so the reads of a level go out together.  A count beyond the tables gets
    // the division in ONE block per level / per backup, which a wave enters only in an episode where `beyond` (below) says
    // that one of its roots can hold such a count.
    auto explore_tab = [&](int a, int cnt1) { return tpdiv[a * (TE + 2) + min(cnt1, TE + 1)]; };
    auto inv_tab = [&](int c) { return rcp[min(c, TE)]; };
    int32_t *path_all = reinterpret_cast<int32_t *>(lds_d + ntab); // [H + 1][waves * 64]  (not in the LDS-resident variant)
    const int ntab2 = (ntab + 1) & ~1;                             // (16-byte alignment of what follows)
    const double *rdict = lds_d + ntab2;                           // LDSR: [n_rdict] distinct rewards
    uint16_t *t16 = reinterpret_cast<uint16_t *>(lds_d + ntab2 + ((p.n_rdict + 1) & ~1)); // LDSR: [S*A] transitions
    uint8_t *r8 = reinterpret_cast<uint8_t *>(t16 + ((p.S * A + 7) & ~7)); // LDSR: [S*A]
    uint32_t *jump = reinterpret_cast<uint32_t *>(r8 + ((p.S * A + 15) & ~15)); // QD: [H + 5][8]
    if (QD)
        for (int i = tid; i < (H + 5) * 8; i += nthreads) jump[i] = p.jump[i];
    // CartPole: the sin / cos table of libm_sincos.hpp, in LDS behind the path stack (the host sizes the allocation)
    double *sctab_lds = reinterpret_cast<double *>(path_all + (((H + 1) * nthreads + 1) & ~1));
    if (CART)
        for (int i = tid; i < MP_SINCOS_ENTRIES; i += nthreads) sctab_lds[i] = kSincosTab[i];
    // CartPole with replicated roots: the generator's jump table behind the sin / cos table
    uint32_t *cjump = reinterpret_cast<uint32_t *>(sctab_lds + MP_SINCOS_ENTRIES); // [H + 5][8]
    if (CART && p.rep_shift >= 2)
        for (int i = tid; i < (H + 5) * 8; i += nthreads) cjump[i] = p.jump[i];
    const double *sctab = CART ? sctab_lds : nullptr;
#ifdef MP_WAVE_STAMPS
    // WAVE STAMPS (diagnostic build, -DMP_WAVE_STAMPS; tools/uct_wave_finish.py): lane 0 of every wave stores the 100 MHz
    // constant clock at entry, after the staging barrier, after its last episode and at exit, and where it runs (HW_ID, XCC_ID),
    // each with a plain vector store at once -- nothing is held in a register.  No stamp executes in the plain build.
    const long stamp_wave = (long)blockIdx.x * p.waves + wave;
    auto wave_stamp = [&](int k) {
        if (p.wave_stamps && lane == 0) p.wave_stamps[stamp_wave * kWaveStampWords + k] = __builtin_amdgcn_s_memrealtime();
    };
    if (p.wave_stamps && lane == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        p.wave_stamps[stamp_wave * kWaveStampWords + 4] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
    }
    wave_stamp(0);
#define WAVE_STAMP(k) wave_stamp(k)
#else
#define WAVE_STAMP(k)
#endif
    for (int i = tid; i < ntab; i += nthreads) lds_d[i] = p.tab[i];
    if (LDSR) {
        for (int i = tid; i < p.n_rdict; i += nthreads) lds_d[ntab2 + i] = p.rdict[i];
        const int n16 = (p.S * A + 15) >> 4; // (the device array is padded to whole 16-byte chunks)
        const uint4 *src = reinterpret_cast<const uint4 *>(p.r8);
        uint4 *dst = reinterpret_cast<uint4 *>(r8);
        for (int i = tid; i < n16; i += nthreads) dst[i] = src[i];
    }
    if (LDSR) {
        // S*A uint16 entries, staged with 16-byte loads where the tail allows
        const int n = p.S * A;
        const int n8 = n >> 3;
        const uint4 *src = reinterpret_cast<const uint4 *>(p.t16);
        uint4 *dst = reinterpret_cast<uint4 *>(t16);
        for (int i = tid; i < n8; i += nthreads) dst[i] = src[i];
        for (int i = (n8 << 3) + tid; i < n; i += nthreads) t16[i] = p.t16[i];
    }
    // ACTION TABLE (profiles/uct_action_table.md; the table: uct_action_table.hpp).  The rollout's policy is state-independent, so
    // a step's action is a function of its draw alone, and for all but at most |A| - 1 of the 4 096 values of the draw's top twelve
    // bits a function of those bits: one byte read from LDS instead of |A| - 1 compares of 64 bits and their adds.  A step in
    // which some lane of the wave draws into a bucket that holds a threshold (kUctActExact) takes the compares for the whole
    // wave, behind a wave-uniform branch.  The read sits one step AHEAD, beside the speculative draw it belongs to and off the
    // state chain: a step is handed its action, not its draw.
    if constexpr (ATAB) {
        const uint4 *src = reinterpret_cast<const uint4 *>(p.act_tab);
        uint4 *dst = reinterpret_cast<uint4 *>(lds_bytes + (BAL ? kUctBalBytes : 0));
        for (int i = tid; i < kUctActBytes / 16; i += nthreads) dst[i] = src[i];
    }
    // WAVE BALANCE (profiles/uct_wave_balance.md; the rule: uct_balance.hpp).  The saturated form runs four waves per SIMD for the
    // whole kernel, in one round, and with equal priorities the SIMD serves the oldest first: the oldest runs its rollouts near the
    // speed of its dependency chain, the youngest gets what is left, and the last wave of every SIMD ends the kernel alone, at
    // half a SIMD's issue rate with every gather exposed.  So each wave keeps a PROGRESS WORD at the start of the LDS -- its
    // episode and the SIMD it runs on, kUctBalGone once it is done or if it has no root -- reads its workgroup's sixteen before each
    // rollout, and runs the rollout at priority 1 if it has a mate on its SIMD and none of them is in an earlier episode, at 0
    // otherwise: the waves that are ahead yield.  Nobody waits for anybody and no result depends on a word.  The word's slot is
    // the wave's number in the launch modulo 16 (a workgroup's waves -- a power of two <= 16 of them -- take distinct slots), which
    // the wave reads off its root index: no register is kept for it.  Here each wave initialises the slots congruent to its own
    // modulo the waves per workgroup (every slot exactly once), before the barrier that publishes the model.
    if constexpr (BAL) {
        const int g0 = blockIdx.x * p.waves + wave;
        const uint32_t mine = (long)g0 * p.lanes < p.n_roots ? uct_bal_word(0, simd_id()) : kUctBalGone;
        if (lane < kUctBalWords && ((lane ^ g0) & (p.waves - 1)) == 0) bal_store(&lds_bal[lane], lane == (g0 & (kUctBalWords - 1)) ? mine : kUctBalGone);
    }
    __syncthreads();
    WAVE_STAMP(1);
    int32_t *path = path_all + wave * 64; // slot d of this lane: path[d * nthreads + lane]
    const int slot = QD ? lane >> 2 : (CART ? lane >> p.rep_shift : lane);   // which root of the wave (QD: four lanes per root, the first one owns it)
    const bool owner = QD ? (lane & 3) == 0 : true;
    const int r = (blockIdx.x * p.waves + wave) * p.lanes + slot;
#ifdef MP_WAVE_STAMPS
    if (slot >= p.lanes || r >= p.n_roots) { WAVE_STAMP(2); WAVE_STAMP(3); }   // (lane 0 leaves only with its whole wave)
#endif
    if (slot >= p.lanes || r >= p.n_roots) return;   // (QD: whole quads leave together; BAL: a wave without roots wrote kUctBalGone above)
    static_assert(IL != 2 || AT > 0, "the group-interleaved layout needs |A| at compile time");
    const TreeRef<IL, AT> tree = tree_of<IL, AT>(p.tree, r, p.cap, A);
    // TREE STORES.  Layout 2 puts group g of a wave's 64 roots in ONE run of 64 x |A| nodes, and every slot of a new group gets the
    // same constant {0.0, 0, -1}: a lane that writes its own |A| nodes makes |A| stores at an |A| x 16 B stride, each lane of each a
    // line request of its own (320 for 40 lines of data at |A| = 5).  WEXP: the WAVE writes the run instead, lane j of store i the
    // element i * 64 + j (TreeRef::handle transposed), masked to the slots whose owner lane expands at that group -- the same bytes
    // as before in |A| coalesced stores (the expansion below).  Only for a wave whose 64 lanes are 64 consecutive live roots
    // (wave_exp: wave-uniform); a tail wave, fewer roots per wave, phantom counts (MK), root-major trees and CartPole keep the
    // per-lane stores.  LEAF1: an expanded node below the root's children gets its first_child with the 16-byte
    // store of its statistics in the backup that follows (it is the first node the backup writes) instead of a 4-byte store of its
    // own at the expansion.  p.tree_stores == 0 (MP_UCT_TREE_STORES=lane) runs the per-lane forms of both: for A/B runs.
    // Which instantiations take part (profiles/uct_tree_stores.md): the wave's stores cost four to six VGPRs, which |A| >= 6 does
    // not have (the gather form would lose its fourth wave per SIMD), and they are for the forms that gather the model from global
    // memory, where they measure 3-5 % -- in the LDS-resident forms, whose env steps make no memory request, they measured as
    // nothing beside the leaf's store, and those keep the per-lane stores.  The leaf's first_child is one more value alive over
    // the rollout, and the LDS-resident form of |A| >= 7 already spills without it.
    constexpr bool WEXP = IL == 2 && AT > 0 && AT <= 5 && !MK && !LDSR && !CART;
    constexpr int WEXP_PASSES = 4;   // wave-wide passes per expansion, one per distinct tree size (fresh trees: 2-4 sizes per wave)
    constexpr bool LEAF1 = AT > 0 && !(LDSR && !QD && AT >= 7);
    const bool leaf1 = LEAF1 && p.tree_stores != 0;
    // VIRGIN GROUPS (profiles/uct_virgin_groups.md).  A node expands on its first visit only, so a node with children and count 1
    // has not been entered since: its children are all {0.0, 0, -1}.  VSKIP: the selection that stands in such a node takes the
    // constant instead of loading the group (kept trees too: a node that expands late there gets count >= 2).  VDEFER, fresh
    // trees only: the expansion stores no zero group at all -- most groups are never entered again -- and the first entry stores
    // the |A| - 1 siblings it does not pick; the picked one is the episode's leaf, which the backup stores whole (LEAF1).  Until
    // then the group's memory holds whatever was there: every reader applies the rule (uct_virgin.hpp; the host marks the trees).
    // p.tree_stores == 2 (MP_UCT_TREE_STORES=virgin; kept trees) runs both, 1 (MP_UCT_TREE_STORES=group) neither.
    // VISITED MASK (profiles/uct_visited_mask.md; uct_virgin.hpp has the rule), fresh trees only, p.tree_stores == 3 (the default).
    // A child that no episode picked is the constant node too, whatever its parent's count, so the siblings of a pick need never
    // be stored: the first_child word of an expanded node carries, above bit 24, which of its children have been.  A descent
    // loads the children whose bit is set, each under its own predicate, and takes the constant for the others (the whole group
    // loaded wherever any bit is set: MP_UCT_MASK_LOADS, an A/B build).  A pick whose bit is clear is
    // the episode's leaf, which the backup stores whole (LEAF1); the descent sets its bit in the parent's word -- a register for the root's
    // children (tf[]), one 4-byte store for a parent below them.  The root's own children live in registers and are all stored at
    // the read-out: its word gets the full mask there.  As with VDEFER, a pick below the levels whose statistics stay in registers
    // is stored at its entry, because the backup reads it back.  The mask rides in words that are registers already (fc, tf[]):
    // nothing more is alive over the rollout.
    // VM is a template argument like BAL: as a run-time flag beside the two above it spilled scalar registers in every
    // LDS-resident instantiation, two vector registers in the headline's, and cost the gather form of |A| = 5 its fourth wave.
    // The host launches the VM instantiation for fresh trees with p.tree_stores == 3 and no other.
    static_assert(!VM || (uct_mask_form(AT, ENV, SP, MK, IL, QD) && LEAF1 && !CART), "the visited mask: the forms of uct_mask_form");
    constexpr bool VMASK = VM;
    constexpr bool VSKIP = !VM && uct_virgin_form(AT, ENV, SP, MK, IL, QD);
    constexpr bool VDEFER = VSKIP && LEAF1;
    const bool vskip = VSKIP && p.tree_stores >= 2;
    const bool vdefer = VDEFER && p.tree_stores == 2 && p.n_nodes_in == nullptr;
    bool wave_exp = false;
    if constexpr (WEXP) {
        const int wave_r0 = (blockIdx.x * p.waves + __builtin_amdgcn_readfirstlane(wave)) * 64;
        wave_exp = p.tree_stores != 0 && p.lanes == 64 && wave_r0 + 64 <= p.n_roots;
    }
    const Rec *__restrict__ rec = p.rec;
    Pcg64 g;
    g.load(p.rng + (long)r * 6);
    // The one-lane table rollout steps its two generator copies as four 32-bit words each (Pcg64W: 8 vector instructions fewer
    // per trip of two env steps; profiles/uct_pcg_words.md).  `g` itself, the tie draws of the selection and every other rollout
    // form keep Pcg64.  -DMP_PCG_WORDS=0 builds the loop on Pcg64 as before, for A/B runs.
    constexpr bool PCGW = MP_PCG_WORDS != 0 && uct_pcg_words_form(AT, ENV, SP, MK, IL, QD);
    using RollGen = typename std::conditional<PCGW, Pcg64W, Pcg64>::type;
    auto roll_gen = [](const Pcg64 &x) { if constexpr (PCGW) return Pcg64W::from(x); else return x; };
    auto roll_gen_commit = [](Pcg64 &x, const RollGen &y) { if constexpr (PCGW) y.state_to(x); else x = y; };
    // THE LEAN TRIP (above).  TERMTAB: bit 15 of a staged record is the terminal flag the model's rule stops on -- terminal[next]
    // with done_on_next, terminal[s] of the state the step leaves without it (uct_term_table.hpp) -- so a step's test is that bit
    // under either rule.  The flag is a function of the state (mp_model_load_table takes terminal[S] and nothing per action), so
    // terminal[s] read off a record of s is what `cur_term` carried: root_term for the first step of a plan or of a kept tree's
    // next plan, the previous record's bit 15 afterwards.
    constexpr bool TERMTAB = uct_term_table_form(ENV, QD);
    constexpr bool LEANI = MP_UCT_LEAN_INDEX != 0 && PCGW && LDSR;
    constexpr bool LEANH = MP_UCT_LEAN_COUNT != 0 && PCGW;
    uint64_t g4_lo = 0, g4_hi = 0;          // QD: inc * G_4, the additive term of a four-step jump of this root's generator
    if (QD || (CART && p.rep_shift >= 2)) g.inc_g4(g4_lo, g4_hi);
    uint64_t g16_lo = 0, g16_hi = 0;        // CartPole, sixteen replicas: inc * G_16
    if (CART && p.rep_shift >= 4) g.inc_g16(g16_lo, g16_hi);
    const int32_t s0 = CART ? 0 : p.root_state[r];
    const int32_t st0 = p.root_steps ? p.root_steps[r] : 0;
    const uint32_t done_bit = p.done_on_next ? 2u : 1u;
    // terminal flag of the root state itself ("source" rule): every record of a state carries it
    const bool root_term = CART ? false : (rec[(long)s0 * A].flags & 1u) != 0;
    double x0[4] = {0.0, 0.0, 0.0, 0.0};
    if (CART) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x0[i] = p.root_x[(long)r * 4 + i];
    }
    // The pipelined CartPole rollouts evaluate the RESTATED sin / cos without its range test (|x| < 0.855: libm_sincos.hpp).  A
    // live step's angle is within the env's threshold, so they are used only where the threshold and every root angle of the wave
    // are inside that range; anything else (a root handed over with the pole already down, a wide threshold) takes the generic
    // rollout, whose cartpole_step tests the range per call.
    const bool cart_flat = CART && p.cp_sincos != SINCOS_DEVICE && p.cp.theta_threshold < 0.8 && !any64(!(fabs(x0[2]) < 0.8));
    int n_nodes = p.n_nodes_in ? p.n_nodes_in[r] : 0; // > 0: tree kept by step_strategy "subtree"
    constexpr int AR = AT > 0 ? AT : 1;
    // RC: the root and its children (node ids 0..A: the root is always the first node to expand, and a re-rooted
    // tree is renumbered breadth-first) live in registers for the whole plan.  Every episode scores the root's
    // children and backs up the root and one of them: keeping them out of memory removes ~7 of the ~31 L2
    // requests an episode makes.  They are written back once, before the plan is read out.
    constexpr bool RC = AT > 0;
    double tv0 = 0.0, tv[AR];   // value of the root / of its children
    int tc0 = 0, tc[AR];        // count
    int tf0 = -1, tf[AR];       // first_child
#pragma unroll
    for (int a = 0; a < AR; ++a) { tv[a] = 0.0; tc[a] = 0; tf[a] = -1; }
    if (n_nodes < 1) {
        // mcts.py:129-130 reset(): fresh root
        UctNode n;
        n.value = 0.0; n.count = 0; n.first_child = -1;
        if (!RC) tree[0] = n;
        n_nodes = 1;
    } else if (RC) {
        const UctNode r0 = tree[0];
        tv0 = r0.value; tc0 = r0.count; tf0 = r0.first_child;
        if (tf0 == 1) {
#pragma unroll
            for (int a = 0; a < AR; ++a) {
                const UctNode ca = tree.child(1, a);
                tv[a] = ca.value; tc[a] = ca.count; tf[a] = ca.first_child;
            }
        }
    }
    double tp0[AR]; // SP: temperature * |A| * prior[s0][a], the root's children
    uint32_t mask0 = 0xffu; // MK: actions the prior policy lists in the root state
    if (MK) mask0 = (p.pol_frec[(size_t)((unsigned)s0 * A) * (1 + NQ32)].y >> 16) & 0xffu;
    const double TA0 = MK ? p.temperature * (double)__popc(mask0) : p.TA;
#pragma unroll
    for (int a = 0; a < AR; ++a) tp0[a] = SP ? TA0 * p.pol_prior[(long)s0 * p.pol_stride + a] : 0.0;
    int steps_taken = 0;
    // statistics of the path nodes at depths 2..5 as read by the selection of this episode (nobody else writes
    // them in between): the backup then needs no read for them (~16 % of the saturated kernel's time was those reads)
    constexpr int KEEP = (AT > 0 && AT <= 5) ? 4 : 2; // register budget: stay within 128 VGPRs (4 waves per SIMD)
    double kv[KEEP];
    int kc[KEEP];
#pragma unroll
    for (int i = 0; i < KEEP; ++i) { kv[i] = 0.0; kc[i] = 0; }
    // where the handles of the path nodes live: a per-lane stack in LDS ([depth][lane]) -- or, when the model fills the
    // LDS (LDSR), registers for depths 1 .. 1 + KEEP and a global spill array beyond (rarely reached: mean depth ~2)
    int ph1 = 0, ph[KEEP];
#pragma unroll
    for (int i = 0; i < KEEP; ++i) ph[i] = 0;
    // (macros, not lambdas: a closure over `ph` keeps a dead copy of the array in scratch memory)
#define PATH_PUT(d_, h_)                                                                        \
    do {                                                                                        \
        const int pd_ = (d_), phv_ = (h_);                                                      \
        if constexpr (!PREG) {                                                                  \
            path[pd_ * nthreads + lane] = phv_;                                                 \
        } else {                                                                                \
            if (pd_ == 1) ph1 = phv_;                                                           \
            _Pragma("unroll") for (int i_ = 0; i_ < KEEP; ++i_) ph[i_] = pd_ == 2 + i_ ? phv_ : ph[i_]; \
            if (pd_ >= 2 + KEEP) p.path_spill[(size_t)pd_ * p.spill_stride + r] = phv_;        \
        }                                                                                       \
    } while (0)
#define PATH_GET(out_, d_)                                                                      \
    do {                                                                                        \
        const int pd_ = (d_);                                                                   \
        if constexpr (!PREG) {                                                                  \
            out_ = path[pd_ * nthreads + lane];                                                 \
        } else {                                                                                \
            int hh_ = pd_ == 0 ? tree.root_handle() : ph1;                                      \
            _Pragma("unroll") for (int i_ = 0; i_ < KEEP; ++i_) hh_ = pd_ == 2 + i_ ? ph[i_] : hh_; \
            if (pd_ >= 2 + KEEP) hh_ = p.path_spill[(size_t)pd_ * p.spill_stride + r];          \
            out_ = hh_;                                                                         \
        }                                                                                       \
    } while (0)

    // WAVE PRIORITY of the saturated form (one-lane LDS-resident model: sixteen waves per CU, four per SIMD, each an in-order
    // stream).  Its tree phases are chains of dependent gathers from the trees in HBM (selection: one per level; backup: a read
    // and one store per node below the kept levels) with little arithmetic between them; its rollouts are arithmetic on LDS.
    // With equal priorities the SIMD serves the oldest wave first, and a wave in a tree phase waits behind its partners'
    // rollout arithmetic before it can issue the few instructions that put its next gather in flight.  Raised priority in the
    // tree phases starts those gathers as early as possible, and the rollouts of the other waves fill the time they take.
    // (Plain bench runs alternating with the parent's library, eight each: priority alone 0.7836 ms per step against 0.7877,
    // ranges overlapping; with the table quotients below 0.7796, ranges apart.  Rollouts at priority 2 instead: slower.
    // profiles/uct_tree_phase.md.)  The other forms run one or two waves per SIMD and keep the default.
    constexpr int TREE_PRIO = LDSR && !QD ? 2 : 0;
#ifdef MP_PROFILE
    long long t_sel = 0, t_expd = 0, t_roll = 0, t_bak = 0, n_sel = 0, n_roll = 0;
    const long long t_all0 = clock64();
#define PROF_T(x) const long long x = clock64()
#else
#define PROF_T(x)
#endif
    for (int ep = 0; ep < E; ++ep) { // mcts.py:179-184
        PROF_T(c0);
        if constexpr (TREE_PRIO > 0) __builtin_amdgcn_s_setprio(TREE_PRIO);
        int32_t s = s0, st = st0;
        double x4[4] = {x0[0], x0[1], x0[2], x0[3]};
        int node = 0, depth = 0;
        bool terminal = false;
        [[maybe_unused]] bool cur_term = root_term; // terminal[s] of the state the next action is taken from (TERMTAB: in the table)
        double total = 0.0;
        uint32_t cur_mask = mask0; // MK: listed actions of the state the descent is in
        if (!RC) PATH_PUT(0, tree.root_handle());
        int hnode = tree.root_handle(); // where `node` lives (TreeRef handle)
        int fc = RC ? tf0 : tree[0].first_child;
        // No node's count exceeds the root's (a backup adds one to every node of a path that starts at the root; re-rooting keeps a
        // subtree as it is), and this episode adds one: while every root of the wave has counted fewer than TE episodes, every
        // quotient of the episode is in the tables -- fresh trees of at most TE episodes never leave them.  Wave-uniform, so what
        // a level and a backup pay for the division is one scalar branch.
        const bool beyond = RC && any64(tc0 >= TE);
        int node_c = 0; // VSKIP: the count of the node the descent stands in (below the root: the picked child's, as read)
        // ---- selection, mcts.py:143-149
        while (owner && depth < H && fc >= 0 && !terminal) {
            // MCTSNode.selection_strategy (mcts.py:275-286): value + temperature*|A|*prior/(count+1);
            // Node.random_argmax (abstract.py:296-311): exact-equality argmax set, uniform draw
            // among >= 2 ties (no draw for a single maximum)
            int act = 0, nfc = -1;
            if (AT > 0) {
                UctNode c[AR];
                bool virgin = false;
                const int fcw = fc; // VMASK: the word as the node holds it, the visited mask above the id (the root's own: plain)
                if (VMASK) fc &= kUctChildBits;
                if (fc == 1) { // the root's children: registers
#pragma unroll
                    for (int a = 0; a < AR; ++a) { c[a].value = tv[a]; c[a].count = tc[a]; c[a].first_child = tf[a]; }
                } else if (VMASK) { // the children that were stored; the others are the constant node
                    UctNode *grp = &tree.child(fc, 0);
#pragma unroll
                    for (int a = 0; a < AR; ++a) {
                        const bool stored = ((fcw >> (kUctMaskShift + a)) & 1) != 0;
                        c[a].value = 0.0; c[a].count = 0; c[a].first_child = -1;
#if MP_UCT_MASK_LOADS
                        if (stored) c[a] = tree.sibling(grp, a);
#else
                        if ((fcw >> kUctMaskShift) != 0) {
                            const UctNode ld = tree.sibling(grp, a);
                            asm volatile("" ::"v"(ld.count)); // (keeps the load where it is: the compiler sinks it below `stored`)
                            if (stored) c[a] = ld;
                        }
#endif
                    }
                } else if (VSKIP && vskip && node_c == 1) { // a virgin group: nothing to load
                    virgin = true;
#pragma unroll
                    for (int a = 0; a < AR; ++a) { c[a].value = 0.0; c[a].count = 0; c[a].first_child = -1; }
                } else {
                    UctNode *grp = &tree.child(fc, 0);
#pragma unroll
                    for (int a = 0; a < AR; ++a) c[a] = tree.sibling(grp, a);
                }
                double sc[AR];
                if (SP) {
                    double tpl[AR];
                    if (depth == 0) {
#pragma unroll
                        for (int a = 0; a < AR; ++a) tpl[a] = tp0[a];
                    } else {
                        const double *pr = p.pol_prior + (long)s * p.pol_stride;
                        const double TAk = MK ? p.temperature * (double)__popc(cur_mask) : p.TA;
#pragma unroll
                        for (int a = 0; a < AR; ++a) tpl[a] = TAk * pr[a];
                    }
#pragma unroll
                    for (int a = 0; a < AR; ++a) {
                        sc[a] = c[a].value + tpl[a] / (double)(c[a].count + 1);
                        if (MK && c[a].count < 0) sc[a] = -INFINITY; // phantom slot: not a child
                    }
                } else {
                    double ex[AR];
#pragma unroll
                    for (int a = 0; a < AR; ++a) ex[a] = explore_tab(a, c[a].count + 1);
                    if (beyond) {
                        // counts beyond the tables: the IEEE division, one child per trip (one division sequence in the code),
                        // kept only where a lane's child needs it
#pragma nounroll
                        for (int b = 0; b < AR; ++b) {
                            int cb = c[0].count;
#pragma unroll
                            for (int a = 1; a < AR; ++a) cb = b == a ? c[a].count : cb;
                            const double q = tp[b] / (double)(cb + 1);
#pragma unroll
                            for (int a = 0; a < AR; ++a) ex[a] = (b == a && cb > TE) ? q : ex[a];
                        }
                    }
#pragma unroll
                    for (int a = 0; a < AR; ++a) sc[a] = c[a].value + ex[a];
                }
                double m = sc[0];
#pragma unroll
                for (int a = 1; a < AR; ++a) m = sc[a] > m ? sc[a] : m;
                int nt = 0;
#pragma unroll
                for (int a = 0; a < AR; ++a) nt += sc[a] == m ? 1 : 0;
                int pick = nt > 1 ? (int)g.below((uint32_t)nt) : 0;
                bool found = false;
                double sel_v = 0.0;
                int sel_c = 0;
#pragma unroll
                for (int a = 0; a < AR; ++a) {
                    const bool eq = sc[a] == m;
                    if (eq && !found && pick == 0) {
                        act = a; nfc = c[a].first_child; found = true;
                        sel_v = c[a].value; sel_c = c[a].count;
                    }
                    if (eq && !found) --pick;
                }
#pragma unroll
                for (int i = 0; i < KEEP; ++i)
                    if (depth + 1 == 2 + i) { kv[i] = sel_v; kc[i] = sel_c; }
                node_c = sel_c;
                if (VDEFER && vdefer && virgin) {
                    // the first entry of a group no expansion stored: the siblings of the pick (the backup stores the pick whole) --
                    // and the pick too where the backup READS a node's statistics back before it stores them (below the levels
                    // whose statistics stay in registers: rare)
                    UctNode z;
                    z.value = 0.0; z.count = 0; z.first_child = -1;
                    UctNode *grp = &tree.child(fc, 0);
                    const bool deep = depth + 1 >= 2 + KEEP;
#pragma unroll
                    for (int a = 0; a < AR; ++a)
                        if (a != act || deep) tree.sibling(grp, a) = z;
                }
                if (VMASK && depth >= 1 && !((fcw >> (kUctMaskShift + act)) & 1)) {
                    // the first pick of a child below the root's: its bit into the parent's word -- tf[] for a child of the
                    // root (node = 1 + its action), else the word in memory (hnode is still the parent's handle).  No sibling is
                    // stored; the pick itself only where the backup reads it back (see VDEFER above)
                    const int w = fcw | (1 << (kUctMaskShift + act));
                    if (depth == 1) {
#pragma unroll
                        for (int a = 0; a < AR; ++a) tf[a] = node == 1 + a ? w : tf[a];
                    } else {
                        tree.at(hnode).first_child = w;
                    }
                    if (depth + 1 >= 2 + KEEP) {
                        UctNode z;
                        z.value = 0.0; z.count = 0; z.first_child = -1;
                        tree.child(fc, act) = z;
                    }
                }
            } else {
                double m = 0.0;
                for (int a = 0; a < A; ++a) {
                    const UctNode c = tree.child(fc, a);
                    const double sc = c.value + explore(a, c.count + 1);
                    if (a == 0 || sc > m) m = sc;
                }
                int nt = 0;
                for (int a = 0; a < A; ++a) {
                    const UctNode c = tree.child(fc, a);
                    nt += (c.value + explore(a, c.count + 1)) == m ? 1 : 0;
                }
                int pick = (int)g.below((uint32_t)nt);
                for (int a = 0; a < A; ++a) {
                    const UctNode c = tree.child(fc, a);
                    if ((c.value + explore(a, c.count + 1)) == m) {
                        if (pick == 0) { act = a; nfc = c.first_child; break; }
                        --pick;
                    }
                }
            }
            const long idx = (long)s * A + act;
            double reward;
            if (CART) {
                terminal = cartpole_step(p.cp, x4, act, p.cp_sincos, sctab);
                reward = 1.0;
            } else if (LDSR) {
                const uint32_t e = t16[idx];
                reward = rdict[r8[idx]];
                const bool next_term = (e & 0x8000u) != 0;
                if constexpr (TERMTAB) {
                    terminal = next_term;   // (bit 15 is the flag of the model's rule: the table staged is the rule's)
                } else {
                    terminal = p.done_on_next ? next_term : cur_term;
                    cur_term = next_term;
                }
                s = (int32_t)(e & 0x7fffu);
            } else if (MK) {
                const uint4 q0 = p.pol_frec[(size_t)idx * (1 + NQ32)]; // the (s, a) record with the policy's masks
                terminal = (q0.y & done_bit) != 0;
                reward = __hiloint2double((int)q0.w, (int)q0.z);
                s = (int32_t)q0.x;
                cur_mask = (q0.y >> 8) & 0xffu;
            } else {
                const Rec rc = rec[idx];
                terminal = (rc.flags & done_bit) != 0;
                reward = rc.reward;
                s = rc.next;
            }
            ++st;
            ++steps_taken;
            total += gpow[depth] * reward;
            node = fc + act;
            hnode = tree.handle(fc, act);
            ++depth;
            PATH_PUT(depth, hnode);
            fc = nfc;
#ifdef MP_PROFILE
            ++n_sel;
#endif
        }
        PROF_T(c1);
        // ---- expansion, mcts.py:151-154 / 237-246
        bool wexp_pend = false; // WEXP: the new group of this lane is still to be written
        if (owner && fc < 0 && depth < H && (!terminal || node == 0)) {
            UctNode n;
            n.value = 0.0; n.count = 0; n.first_child = -1;
            if (RC && node <= A) {
                if (node == 0) tf0 = n_nodes;
#pragma unroll
                for (int a = 0; a < AR; ++a) tf[a] = node == 1 + a ? n_nodes : tf[a];
            } else if (!leaf1) {
                tree.at(hnode).first_child = n_nodes;
            }
            if (LEAF1) fc = n_nodes; // first_child of the leaf, for the backup's store of it (unchanged where nothing expands)
            if (MK) {
                if (node == 0) {
#pragma unroll
                    for (int a = 0; a < AR; ++a) tc[a] = (cur_mask >> a) & 1u ? 0 : -1;
                } else {
                    UctNode *grp = &tree.child(n_nodes, 0);
                    for (int a = 0; a < A; ++a) {
                        n.count = (cur_mask >> a) & 1u ? 0 : -1;
                        tree.sibling(grp, a) = n;
                    }
                }
            } else if ((VDEFER && vdefer) || VMASK) {
                // (no zero group: the selection that enters it first completes it -- VMASK: nobody does, the new word's mask is 0)
            } else if (!(RC && node == 0)) { // the root's children were zero-initialised in registers
                if constexpr (WEXP) {
                    wexp_pend = true;
                } else {
                    UctNode *grp = &tree.child(n_nodes, 0);
                    if (AT > 0) {
#pragma unroll
                        for (int a = 0; a < AR; ++a) tree.sibling(grp, a) = n;
                    } else {
                        for (int a = 0; a < A; ++a) tree.sibling(grp, a) = n;
                    }
                }
            }
            n_nodes += A;
        }
        if constexpr (WEXP) {
            // the new groups, outside the divergent test.  A wave-wide pass per distinct tree size v among the expanding lanes: the
            // lanes M that expand at v own the slots [l |A|, (l + 1) |A|) of the run of group v, and lane j writes element
            // e = i * 64 + j in store i if its owner e / |A| is in M -- no other lane's group is touched, and the 64-block is
            // allocated whole.  Kept trees can hold 64 sizes: after WEXP_PASSES passes the remaining lanes write their own group.
            UctNode n;
            n.value = 0.0; n.count = 0; n.first_child = -1;
            const int grp_id = n_nodes - AT; // (of a lane that expanded: the first id of its new group)
            if (wave_exp) {
                unsigned long long rem = ballot64(wexp_pend);
                for (int pass = 0; pass < WEXP_PASSES && rem != 0ull; ++pass) {
                    const int v = __builtin_amdgcn_readlane(grp_id, __ffsll((long long)rem) - 1);
                    const bool mine = wexp_pend && grp_id == v;
                    const unsigned long long M = ballot64(mine);
                    const uint32_t m_lo = (uint32_t)M, m_hi = (uint32_t)(M >> 32);
                    // (the lane's number from the count of lanes below it: `lane` itself need not stay in a register for this)
                    const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    UctNode *run = tree.base - ln * AT + (unsigned)((v - 1 + AT) << 6); // (r & 63 == lane in a full wave)
#pragma nounroll
                    for (int i = 0; i < AT; ++i) {
                        const unsigned e = (unsigned)(i * 64 + ln), q = e / (unsigned)AT;
                        if ((((q & 32u) ? m_hi : m_lo) >> (q & 31u)) & 1u) run[e] = n;
                    }
                    wexp_pend = wexp_pend && !mine;
                    rem &= ~M;
                }
                // A group is read back by its owner lane, not by the lanes that stored it.  Both are lanes of ONE wave, whose vector-
                // memory operations reach the L1 in issue order, and no other wave reads these bytes during the kernel: what is needed
                // is that the compiler keeps the order -- a release at wavefront scope (no instruction).
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            }
            if (wexp_pend) {
                UctNode *grp = &tree.child(grp_id, 0);
#pragma unroll
                for (int a = 0; a < AR; ++a) tree.sibling(grp, a) = n;
            }
        }
        if constexpr (BAL) {
            // WAVE BALANCE: publish this wave's episode, read the workgroup's words, pick the rollout's priority.  Lane 0 holds the
            // wave's lowest root, so it is live in every wave that plans, and a wave's live lanes are its first ones: lane j reads word
            // j mod 16.  A tail wave of fewer than sixteen lanes sees the words of its first waves only and may then take priority 1
            // with a mate behind it: one wave of a launch at most, and the words decide nothing but a priority.
            // The wave's own word is its episode counter and remembers its SIMD: the next episode is the word + 4, and neither `ep`
            // nor the SIMD's number is asked for again.
            // (64 roots per wave in this form: r >> 6 is the wave's number in the launch)
            const uint32_t me = __builtin_amdgcn_readfirstlane((uint32_t)r >> 6) & (kUctBalWords - 1);
            const uint32_t mine = __builtin_amdgcn_readfirstlane(bal_load(&lds_bal[me])) + 4u;
            // (the lane's number, asked for here each time: as plain C++ it is loop-invariant, and the compiler keeps it and the mask
            // of lane 0 in registers over the whole plan -- two scalar registers that the |A| = 5 kernel does not have)
            uint32_t ln;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
            const uint32_t j = ln & (kUctBalWords - 1);
            if (ln == 0u) bal_store(&lds_bal[me], mine);
            const uint32_t w = bal_load(&lds_bal[j]);
            const bool other = j != me;
            const uint32_t mates = (uint32_t)ballot64(other & uct_bal_mate(mine, w));
            const uint32_t behind = (uint32_t)ballot64(other & uct_bal_behind(mine, w));
            if ((mates != 0u) & (behind == 0u)) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        } else if constexpr (TREE_PRIO > 0) {
            __builtin_amdgcn_s_setprio(0);
        }
        PROF_T(c2);
        // ---- rollout, mcts.py:156-157 / 160-177.  Two steps per trip over two generator copies (ga, gb):
        // step "a" consumes the draw in `u`, advances gb = next(ga) speculatively while its lookup is in flight
        // and commits it only if the rollout continues; step "b" mirrors it.  No register copies per step,
        // and a rollout that stops leaves the stream exactly where the reference's would be.  In the LDS
        // variant the reward of a step (HBM/L2, off the state chain) is added one step later, in order.
        if constexpr (QD) {
            // ---- rollout, four lanes per root (see the comment on QD above)
            const bool want = owner && !terminal && depth < H;
            if (__any(want ? 1 : 0)) {
                auto bcastq = [](uint32_t v, int q) { // lane q of the quad, to its four lanes (quad_perm q,q,q,q)
                    return (uint32_t)(q == 0 ? __builtin_amdgcn_mov_dpp((int)v, 0x00, 0xf, 0xf, true)
                                             : (q == 1 ? __builtin_amdgcn_mov_dpp((int)v, 0x55, 0xf, 0xf, true)
                                                       : (q == 2 ? __builtin_amdgcn_mov_dpp((int)v, 0xaa, 0xf, 0xf, true)
                                                                 : __builtin_amdgcn_mov_dpp((int)v, 0xff, 0xf, 0xf, true))));
                };
                // the owner's generator state, to the four lanes of its quad; lane j jumps j + 1 steps ahead (draw k of the
                // rollout is the output of the state after k + 1 steps) -- one table-driven jump, not j + 1 steps
                Pcg64 q = g;
                q.s_lo = (uint64_t)bcastq((uint32_t)g.s_lo, 0) | ((uint64_t)bcastq((uint32_t)(g.s_lo >> 32), 0) << 32);
                q.s_hi = (uint64_t)bcastq((uint32_t)g.s_hi, 0) | ((uint64_t)bcastq((uint32_t)(g.s_hi >> 32), 0) << 32);
                const uint64_t st_lo = q.s_lo, st_hi = q.s_hi;      // (the state the final jump by n starts from)
                {
                    const int j1 = (lane & 3) + 1;
                    uint32_t an[4], gn[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { an[i] = jump[j1 * 8 + i]; gn[i] = jump[j1 * 8 + 4 + i]; }
                    q.jump(an, gn);
                }
                auto draw = [&](const Pcg64 &gen) -> uint32_t {     // searchsorted(cdf, u, 'right') on the raw 64-bit output
                    const uint64_t u = gen.output();
                    int act = 0;
#pragma unroll
                    for (int a = 0; a < NTH; ++a) act += p.thr_arg[a] <= u ? 1 : 0;
                    return (uint32_t)min(act, p.thr_valid);
                };
                // ROUNDS of four draws (one per lane) and four steps of the owner's walk, as long as any root of the wave is
                // still rolling; the draws of round r + 1 are computed beside the walk of round r (independent instruction
                // streams of one basic block: the walk's LDS round trips hide under the generator's multiplies).  Every step is
                // unconditional arithmetic with selects -- a finished root re-reads a valid record and keeps its values.
                // (round 6, as uct_row_kernel's walk) a round in two passes: the state chain alone -- index -> LDS read -> mask, SPECULATIVE
                // past the rollout's end (valid records nobody uses) -- with the rewards' reads beside it; then the round's bookkeeping as
                // bit arithmetic: stop bit j = "the rollout ends AFTER step j", steps taken = first stop bit + 1 (or 4); a step not taken
                // adds +0.0 to a return that is never -0.  The step counters advance once, after the rollout.
                bool alive = want;
                int h = depth;
                const int hmax = p.max_steps > 0 ? min(H, depth + p.max_steps - st) : H;   // (the first step is unconditional)
                uint32_t act_cur = draw(q);
                q.advance4(g4_lo, g4_hi);
                while (__any(alive ? 1 : 0)) {
                    const uint32_t a4[4] = {bcastq(act_cur, 0), bcastq(act_cur, 1), bcastq(act_cur, 2), bcastq(act_cur, 3)};
                    const uint32_t act_next = draw(q);
                    q.advance4(g4_lo, g4_hi);
                    uint32_t e4[4];
                    double rw4[4];
                    int32_t sw = s;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned idx = (unsigned)(sw * A) + a4[i];
                        e4[i] = t16[idx];
                        rw4[i] = rdict[r8[idx]];
                        sw = (int32_t)(e4[i] & 0x7fffu);
                    }
                    const uint32_t nt = ((e4[0] >> 15) & 1u) | ((e4[1] >> 14) & 2u) | ((e4[2] >> 13) & 4u) | ((e4[3] >> 12) & 8u);
                    const uint32_t th = p.done_on_next ? nt : (((nt << 1) | (cur_term ? 1u : 0u)) & 15u);
                    const int left = hmax - h;                      // steps still allowed (the first one always is)
                    const uint32_t lim = left <= 4 ? 1u << ((max(left, 1) - 1) & 3) : 0u;
                    const uint32_t stop = th | lim;
                    const int first = stop ? __ffs((int)stop) - 1 : 4;
                    const int k = alive ? min(first + 1, 4) : 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double add = gpow[min(h + j, H)] * rw4[j];
                        total += j < k ? add : 0.0;
                    }
                    const uint32_t ek = k <= 1 ? e4[0] : (k == 2 ? e4[1] : (k == 3 ? e4[2] : e4[3]));
                    s = k > 0 ? (int32_t)(ek & 0x7fffu) : s;
                    cur_term = k > 0 ? (ek & 0x8000u) != 0 : cur_term;
                    h += k;
                    alive = alive && first >= 4;
                    act_cur = act_next;
                }
                const int n = h - depth;
                st += n; steps_taken += n;
                if (want) { // the generator after the n draws the walk consumed: A^n state + inc G_n
                    uint32_t an[4], gn[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { an[i] = jump[n * 8 + i]; gn[i] = jump[n * 8 + 4 + i]; }
                    g.s_lo = st_lo; g.s_hi = st_hi;
                    g.jump(an, gn);
                }
            }
        } else
        if (CART && cart_flat && p.rep_shift >= 2) {
            // ---- CartPole rollout, REPLICATED ROOTS (round 6).  The launch code gives a root 2^rep_shift >= 4 lanes that all compute
            // the same plan (why: see there).  What the replicas can do differently is numpy's generator: the action sequence of a
            // rollout does not depend on the states it visits (uniform policy), so lane j of a quad holds the generator j + 1 steps
            // ahead and jumps by four per round (as the four-lanes-per-root table kernel, QD above): a step takes its force from a
            // quad broadcast, and the 128-bit generator step is executed once per FOUR env steps.  The rollout is software-pipelined
            // as the one-lane form below (sin / cos of the next angle beside this step's accelerations).  The walk consumes n draws; the
            // generator then jumps by exactly n.  The three divisions by the constant total mass take the short exact form (div_by_const; FD below).  Every value is cartpole_step's, operation for operation (same bits: tests/test_gpu_cartpole.py).
            bool alive = !terminal && depth < H;
            if (any64(alive)) {
                const mp_cartpole_params &c = p.cp;
                const double total_mass = c.masspole + c.masscart, polemass_length = c.masspole * c.length;
                const double inv_tm = p.cp_inv_tm;
                // FD: the three divisions by the constant total mass as div_by_const (24 vector instructions fewer per step: 0.336 ->
                // 0.298 ms).  Its numerators stay in {0} U [2^-960, 2^1000] while the pole's angular velocity stays below 2^300 with
                // parameters in [2^-50, 2^50] (host check): |a1| = |force + pml thd^2 sn| <= 2^701 and is 0 or >= ulp(force) / 2;
                // masspole cs^2 >= 2^-52 for a live angle; |thetaacc| <= 2^752 / den_min <= 2^802, so |a3| = |pml thetaacc cs| <=
                // 2^902, and a3 is 0 or >= 2^-901 (thetaacc = num / den with num = g sn - cs temp: 0, or >= 2^-209 when a1 != 0, or
                // = g sn >= 2^-747 when a1 = 0, which needs |sn| >= 2^-697 under the velocity bound).  The rollout tracks max |thd|
                // (one v_max_f64 per step, finished roots included: their values stay finite) and is REDONE with IEEE divisions if
                // the bound failed or the velocity is not a number -- nothing is committed before.
                // RL: draws per round = lanes of a root that hold the generator at consecutive steps -- 4 (a quad) or, with sixteen
                // replicas, 16 (a DPP row: the generator step once per SIXTEEN env steps)
                auto roll = [&](auto fma_tag, auto fd_tag, auto rl_tag, bool alive) -> bool {   // (`alive` by value: a redo starts from the same state)
                constexpr bool FMA_FORM = decltype(fma_tag)::value, FD = decltype(fd_tag)::value;
                constexpr int RL = decltype(rl_tag)::value;
                auto divc = [&](double a) -> double {
                    if constexpr (FD) return div_by_const(a, total_mass, inv_tm);
                    else return a / total_mass;
                };
                const bool want = alive;
                const uint64_t st_lo = g.s_lo, st_hi = g.s_hi;      // (the state the final jump by n starts from)
                Pcg64 q = g;
                {
                    const int j1 = min((lane & (RL - 1)) + 1, H);     // (draws beyond the horizon are never used)
                    uint32_t an[4], gn[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { an[i] = cjump[j1 * 8 + i]; gn[i] = cjump[j1 * 8 + 4 + i]; }
                    q.jump(an, gn);
                }
                auto next_round = [&] { if constexpr (RL == 16) q.advance16(g16_lo, g16_hi); else q.advance4(g4_lo, g4_hi); };
                // the high word of the force this lane's draw selects (+- force_mag differ in the sign bit only)
                const int f_lo = __double2loint(c.force_mag);
                const uint32_t f_pos = (uint32_t)__double2hiint(c.force_mag), f_neg = (uint32_t)__double2hiint(-c.force_mag);
                auto force_hi = [&](const Pcg64 &gen) -> uint32_t {
                    const uint64_t u = gen.output();
                    int act = 0;
#pragma unroll
                    for (int a = 0; a < NTH; ++a) act += p.thr_arg[a] <= u ? 1 : 0; // scalar operands (RAWU: the raw 64-bit draw)
                    act = min(act, p.thr_valid);
                    return act == 1 ? f_pos : f_neg;
                };
                uint32_t f_cur = force_hi(q);
                next_round();
                int h = depth;
                // the step after which the rollout stops at the latest: the horizon, or the environment's step limit
                const int hmax = p.max_steps > 0 ? min(H, depth + p.max_steps - st) : H;
                double x = x4[0], x_dot = x4[1], theta = x4[2], theta_dot = x4[3];
                double sn, cs;
                libm_sincos_small_flat<FMA_FORM>(theta, &sn, &cs, sctab);
                // BRANCH-FREE steps: a lane whose rollout ended keeps stepping on values nobody reads (only its return, its step
                // count and `alive` are frozen), so a round of four steps is one basic block for the scheduler to interleave.
                double ret = total;
                double vmax = fabs(theta_dot);             // FD: the largest |angular velocity| a division of this rollout saw
                // The same step with its instruction stream ORDERED BY HAND (FMA form of the host libm + the short exact divisions: what
                // an MI355X host runs).  A lone wave issues in order -- a dependent f64 instruction ~10 cycles after its producer, an
                // independent one after ~5 (tools/ilp_rate.hip) -- and the compiler emits the step's chains one after the other
                // (profiles/r06_cartpole.md).  Here the chains are written side by side, one operation of each per group, and an EMPTY
                // asm volatile that "modifies" the group's results ties them together: the next operation of every chain then has to be
                // emitted after it (a scheduling barrier alone does not do it: instruction selection linearises the block chain by chain
                // before the machine scheduler sees the barrier).  The chains: the velocity recurrence (a1 -> temp -> num -> thetaacc),
                // the other divisor (masspole cs^2 / m -> den), sin's Taylor polynomial and the table path of sin / cos of the NEXT
                // angle, then the IEEE division (the compiler's own sequence, spelled out) beside the table path's corrections, then the
                // last short division beside the bookkeeping.  Operation for operation the arithmetic of one_step below (which stays
                // for the other forms): the same bits.
#define MP_T2(a, b) asm volatile("" : "+v"(a), "+v"(b))
#define MP_T3(a, b, c_) asm volatile("" : "+v"(a), "+v"(b), "+v"(c_))
#define MP_T4(a, b, c_, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c_), "+v"(d))
#define MP_T5(a, b, c_, d, e) asm volatile("" : "+v"(a), "+v"(b), "+v"(c_), "+v"(d), "+v"(e))
                auto one_step_il = [&](uint32_t f_hi) {
                    typedef LibmConst K;
                    const double m = total_mass, y = inv_tm;
                    const double force = __hiloint2double((int)f_hi, f_lo);
                    double txd = c.tau * x_dot, tthd = c.tau * theta_dot, thd2 = theta_dot * theta_dot, cs2 = cs * cs;
                    MP_T4(txd, tthd, thd2, cs2);
                    double x_n = x + txd, th_n = theta + tthd, t2 = polemass_length * thd2, a2 = c.masspole * cs2, gsn = c.gravity * sn;
                    MP_T5(x_n, th_n, t2, a2, gsn);
                    const double ax = fabs(th_n);
                    double u = K::big + ax, t3 = t2 * sn, qa0 = a2 * y, xxt = th_n * th_n;
                    MP_T4(u, t3, qa0, xxt);
                    double ub = u - K::big, a1 = force + t3, ra0 = __fma_rn(-qa0, m, a2), pt = __fma_rn(xxt, K::s5, K::s4);
                    int i4 = libm_low_word(u) << 2;
                    i4 = i4 < 0 ? 0 : (i4 > MP_SINCOS_ENTRIES - 4 ? MP_SINCOS_ENTRIES - 4 : i4);
                    const double tsn = sctab[i4], tssn = sctab[i4 + 1], tcs = sctab[i4 + 2], tccs = sctab[i4 + 3];
                    const double gp = gpow[h];
                    MP_T4(ub, a1, ra0, pt);
                    double r = ax - ub, q0 = a1 * y, qa1 = __fma_rn(ra0, y, qa0);
                    pt = __fma_rn(xxt, pt, K::s3);
                    MP_T4(r, q0, qa1, pt);
                    double xx = r * r, r0m = __fma_rn(-q0, m, a1), ra1 = __fma_rn(-qa1, m, a2);
                    pt = __fma_rn(xxt, pt, K::s2);
                    MP_T4(xx, r0m, ra1, pt);
                    double rxx = r * xx, pp = __fma_rn(xx, K::sn5, K::sn3), q1 = __fma_rn(r0m, y, q0), a2q = __fma_rn(ra1, y, qa1);
                    pt = __fma_rn(xxt, pt, K::s1);
                    MP_T5(rxx, pp, q1, a2q, pt);
                    double qq = __fma_rn(xx, K::cs6, K::cs4), r1m = __fma_rn(-q1, m, a1), dd = 4.0 / 3.0 - a2q, tt = __fma_rn(th_n, pt, -0.0);
                    const double dxs = th_n <= 0 ? -0.0 : 0.0;
                    MP_T4(qq, r1m, dd, tt);
                    qq = __fma_rn(xx, qq, K::cs2);
                    double s_cos = __fma_rn(rxx, pp, r), temp = __fma_rn(r1m, y, q1), den = c.length * dd;
                    tt = __fma_rn(tt, xxt, 0.0);
                    MP_T5(qq, s_cos, temp, den, tt);
                    double cc = xx * qq, ssi = __fma_rn(rxx, pp, dxs), cst = cs * temp, sin_taylor = th_n + tt;
                    MP_T4(cc, ssi, cst, sin_taylor);
                    double s_sin = r + ssi, num = gsn - cst;
                    MP_T2(s_sin, num);
                    // thetaacc = num / den: v_div_scale x 2, v_rcp, two refinements, quotient, residual, v_div_fmas, v_div_fixup
                    bool fl0, fl1;
                    double d0 = __builtin_amdgcn_div_scale(num, den, false, &fl0);
                    double e1s = __fma_rn(s_sin, tccs, tssn), e1c = __fma_rn(-s_cos, tssn, tccs);
                    MP_T3(d0, e1s, e1c);
                    double d1 = __builtin_amdgcn_div_scale(num, den, true, &fl1);
                    double rr = __builtin_amdgcn_rcp(d0);
                    double e2s = __fma_rn(-cc, tsn, e1s), e2c = __fma_rn(-cc, tcs, e1c);
                    MP_T4(d1, rr, e2s, e2c);
                    double ea = __fma_rn(-d0, rr, 1.0), cor_s = __fma_rn(s_sin, tcs, e2s), cor_c = __fma_rn(-s_cos, tsn, e2c);
                    MP_T3(ea, cor_s, cor_c);
                    rr = __fma_rn(rr, ea, rr);
                    double sin_tab0 = tsn + cor_s, cs_n = tcs + cor_c;
                    MP_T3(rr, sin_tab0, cs_n);
                    double eb = __fma_rn(-d0, rr, 1.0), sin_tab = copysign(sin_tab0, th_n);
                    const bool fell = fabs(x_n) > c.x_threshold || fabs(th_n) > c.theta_threshold;
                    MP_T2(eb, sin_tab);
                    rr = __fma_rn(rr, eb, rr);
                    double sn_n = libm_select(libm_high_abs(th_n) < 0x3e500000u, th_n, libm_select(ax < 0.126, sin_taylor, sin_tab));
                    MP_T2(rr, sn_n);
                    double qd = d1 * rr;
                    ret = libm_select(alive, ret + gp * 1.0, ret);
                    MP_T2(qd, ret);
                    double ec = __fma_rn(-d0, qd, d1);
                    h += alive ? 1 : 0;
                    alive = alive && !(fell || h >= hmax);
                    double qf = __builtin_amdgcn_div_fmas(ec, rr, qd, fl1);
                    const double thetaacc = __builtin_amdgcn_div_fixup(qf, den, num);
                    double a3a = polemass_length * thetaacc, tth = c.tau * thetaacc;
                    MP_T2(a3a, tth);
                    double a3 = a3a * cs, thd_n = theta_dot + tth;
                    MP_T2(a3, thd_n);
                    const double q30 = a3 * y;
                    vmax = fmax(vmax, fabs(thd_n));
                    const double r30 = __fma_rn(-q30, m, a3);
                    const double q31 = __fma_rn(r30, y, q30);
                    const double r31 = __fma_rn(-q31, m, a3);
                    const double q3 = __fma_rn(r31, y, q31);
                    const double xacc = temp - q3;
                    const double txa = c.tau * xacc;
                    x = x_n; theta = th_n;
                    x_dot = x_dot + txa;
                    theta_dot = thd_n;
                    sn = sn_n; cs = cs_n;
                };
#undef MP_T2
#undef MP_T3
#undef MP_T4
#undef MP_T5
                auto one_step = [&](uint32_t f_hi) {
                    const double force = __hiloint2double((int)f_hi, f_lo);
                    // chain 1: the new positions, then the sin / cos the NEXT step needs
                    const double x_n = x + c.tau * x_dot;
                    const double theta_n = theta + c.tau * theta_dot;
                    double sn_n, cs_n;
                    libm_sincos_small_flat<FMA_FORM>(theta_n, &sn_n, &cs_n, sctab);
                    // chain 2: this step's accelerations from sin / cos of the CURRENT angle
                    const double a1 = force + polemass_length * (theta_dot * theta_dot) * sn;
                    const double temp = divc(a1);
                    const double thetaacc = (c.gravity * sn - cs * temp) / (c.length * (4.0 / 3.0 - divc(c.masspole * (cs * cs))));
                    const double xacc = temp - divc(polemass_length * thetaacc * cs);
                    const double gp = gpow[h];
                    // (x < -T || x > T is |x| > T for every T, NaN included: two compares instead of four)
                    const bool fell = fabs(x_n) > c.x_threshold || fabs(theta_n) > c.theta_threshold;
                    x = x_n; theta = theta_n;
                    x_dot = x_dot + c.tau * xacc;
                    theta_dot = theta_dot + c.tau * thetaacc;
                    if constexpr (FD) vmax = fmax(vmax, fabs(theta_dot));
                    sn = sn_n; cs = cs_n;
                    ret = libm_select(alive, ret + gp * 1.0, ret);
                    h += alive ? 1 : 0;
#ifdef MP_PROFILE
                    n_roll += alive ? 1 : 0;
#endif
                    alive = alive && !(fell || h >= hmax);
                };
                auto step = [&](uint32_t f_hi) {
#ifndef MP_CART_NO_IL
                    if constexpr (FMA_FORM && FD) one_step_il(f_hi); else one_step(f_hi);
#else
                    one_step(f_hi);
#endif
                };
                while (true) {
                    const uint32_t f_next = force_hi(q);
                    next_round();
                    if constexpr (RL == 4) {
                        step(quad_bcast<0>(f_cur)); step(quad_bcast<1>(f_cur)); step(quad_bcast<2>(f_cur)); step(quad_bcast<3>(f_cur));
                    } else {
                        // (the test "is every root of the wave done" after every four steps, as with quads)
                        step(row_bcast<0>(f_cur)); step(row_bcast<1>(f_cur)); step(row_bcast<2>(f_cur)); step(row_bcast<3>(f_cur));
                        if (any64(alive)) {
                            step(row_bcast<4>(f_cur)); step(row_bcast<5>(f_cur)); step(row_bcast<6>(f_cur)); step(row_bcast<7>(f_cur));
                            if (any64(alive)) {
                                step(row_bcast<8>(f_cur)); step(row_bcast<9>(f_cur)); step(row_bcast<10>(f_cur)); step(row_bcast<11>(f_cur));
                                if (any64(alive)) {
                                    step(row_bcast<12>(f_cur)); step(row_bcast<13>(f_cur)); step(row_bcast<14>(f_cur)); step(row_bcast<15>(f_cur));
                                }
                            }
                        }
                    }
                    f_cur = f_next;
                    if (!any64(alive)) break;
                }
                if constexpr (FD)
                    if (any64(want && (!(vmax <= 0x1p300) || theta_dot != theta_dot))) return false;   // (the IEEE form runs it again)
                total = ret;
                const int n = h - depth;                   // env steps = draws of this rollout
                st += n; steps_taken += n;
                if (want) { // the generator after the n draws the walk consumed: A^n state + inc G_n
                    uint32_t an[4], gn[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) { an[i] = cjump[n * 8 + i]; gn[i] = cjump[n * 8 + 4 + i]; }
                    g.s_lo = st_lo; g.s_hi = st_hi;
                    g.jump(an, gn);
                }
                return true;
                };
                auto run = [&](auto fma_tag, auto rl_tag) {
                    if (!p.cp_fastdiv || !roll(fma_tag, std::true_type{}, rl_tag, alive)) roll(fma_tag, std::false_type{}, rl_tag, alive);
                };
                typedef std::integral_constant<int, 4> R4;
                typedef std::integral_constant<int, 16> R16;
                if (p.cp_sincos == SINCOS_LIBM_FMA) { if (p.rep_shift >= 4) run(std::true_type{}, R16{}); else run(std::true_type{}, R4{}); }
                else { if (p.rep_shift >= 4) run(std::false_type{}, R16{}); else run(std::false_type{}, R4{}); }
            }
        } else
        if (CART && cart_flat) {
            // ---- CartPole rollout, SOFTWARE-PIPELINED (round 6).  A step's new positions depend on the OLD state only
            // (x + tau x_dot, theta + tau theta_dot), so the sin / cos of the NEXT angle can be evaluated while this step's
            // accelerations -- three IEEE divisions on the velocity chain -- are: two independent dependency chains in one basic
            // block, which the scheduler interleaves (the restated sin / cos is branch-free for that: libm_sincos_small_flat).  A
            // lone wave runs at the latency of its chain: the chain per step was sin / cos + the accelerations, it is now the
            // longer of the two.  The next draw is computed beside them as well and kept only if the rollout continues.  The
            // arithmetic of every value is cartpole_step's, operation for operation (same bits: tests/test_gpu_cartpole.py).
            bool alive = !terminal && depth < H;
            if (any64(alive)) {
                const mp_cartpole_params &c = p.cp;
                const double total_mass = c.masspole + c.masscart, polemass_length = c.masspole * c.length;
                // (the form of the host libm's sin / cos is a compile-time parameter of the loop: a run-time test inside it would
                // split the step into several basic blocks)
                auto roll = [&](auto fma_tag) {
                constexpr bool FMA_FORM = decltype(fma_tag)::value;
                int h = depth;
                double x = x4[0], x_dot = x4[1], theta = x4[2], theta_dot = x4[3];
                double sn, cs;
                libm_sincos_small_flat<FMA_FORM>(theta, &sn, &cs, sctab);
                Pcg64 gr = g;
                uint64_t u = gr.next64();
                while (true) {
                    int act = 0;
#pragma unroll
                    for (int a = 0; a < NTH; ++a) act += p.thr_arg[a] <= u ? 1 : 0; // scalar operands (RAWU: the raw 64-bit draw)
                    act = min(act, p.thr_valid);
                    const double force = act == 1 ? c.force_mag : -c.force_mag;
                    // chain 1: the new positions, then the sin / cos the NEXT step needs
                    const double x_n = x + c.tau * x_dot;
                    const double theta_n = theta + c.tau * theta_dot;
                    double sn_n, cs_n;
                    libm_sincos_small_flat<FMA_FORM>(theta_n, &sn_n, &cs_n, sctab);
                    // chain 2: this step's accelerations from sin / cos of the CURRENT angle
                    const double temp = (force + polemass_length * (theta_dot * theta_dot) * sn) / total_mass;
                    const double thetaacc = (c.gravity * sn - cs * temp) / (c.length * (4.0 / 3.0 - c.masspole * (cs * cs) / total_mass));
                    const double xacc = temp - polemass_length * thetaacc * cs / total_mass;
                    // chain 3: the next draw, kept only if the rollout continues
                    Pcg64 gs = gr;
                    const uint64_t un = gs.next64();
                    const double gp = gpow[h];
                    const bool fell = x_n < -c.x_threshold || x_n > c.x_threshold || theta_n < -c.theta_threshold || theta_n > c.theta_threshold;
                    if (alive) {
                        x = x_n; theta = theta_n;
                        x_dot = x_dot + c.tau * xacc;
                        theta_dot = theta_dot + c.tau * thetaacc;
                        sn = sn_n; cs = cs_n;
                        total += gp * 1.0;
                        ++st; ++steps_taken; ++h;
#ifdef MP_PROFILE
                        ++n_roll;
#endif
                        alive = !(fell || (p.max_steps > 0 && st >= p.max_steps) || h >= H);
                        if (alive) { gr = gs; u = un; }
                    }
                    if (!any64(alive)) break;
                }
                if (!terminal && depth < H) g = gr; // the generator whose draw was consumed last
                };
                if (p.cp_sincos == SINCOS_LIBM_FMA) roll(std::true_type{});
                else roll(std::false_type{});
            }
        } else
        if (!terminal && depth < H) {
            int h = depth;
            // the step after which the rollout stops at the latest: the horizon, or the environment's step limit (the first step
            // is unconditional, as in the reference's loop: hmax <= depth stops after it)
            const int hmax = p.max_steps > 0 ? min(H, depth + p.max_steps - st) : H;
            RollGen ga = roll_gen(g), gb = ga;
            uint64_t u = ga.next64() >> USH; // the 53 random bits of Generator.random() (RAWU: all 64, see thr_arg)
            // ATAB: the action of a draw from its bucket's byte; the exact compares, clamp included, for every lane of the wave in
            // a step where any of them reads kUctActExact (a scalar branch: a per-lane test is if-converted and both paths run)
            [[maybe_unused]] auto table_action = [&](uint64_t draw) -> uint32_t {
                uint32_t t = lds_act[(uint32_t)(draw >> (64 - kUctActBits))];
                if (any64(t > (uint32_t)NTH)) {
                    int act = 0;
#pragma unroll
                    for (int a = 0; a < NTH; ++a) act += p.thr_arg[a] <= draw ? 1 : 0; // scalar operands
                    t = (uint32_t)min(act, p.thr_valid);
                }
                return t;
            };
            uint32_t act_next = 0;           // ATAB: the action of the step to come (that of the draw in `u`)
            if constexpr (ATAB) act_next = table_action(u);
            bool stopped_in_a = true;
            double r_a = 0.0, r_b = 0.0, g_a = 0.0, g_b = 0.0;
            bool have_b = false;
            uint32_t tcur[NTH]; // SP: top 32 bits of the thresholds of the state the rollout is in (saturated)
            if (SP) {
                const uint4 *tr = reinterpret_cast<const uint4 *>(p.pol_thr + (long)s * p.pol_stride);
                const int shift = p.pol_shift;
                const uint64_t sat = p.pol_sat;
                auto coarse = [shift, sat](uint32_t lo, uint32_t hi) { // min(thr >> shift, sat)
                    const uint64_t c = (((uint64_t)hi << 32) | lo) >> shift;
                    return c > sat ? (uint32_t)sat : (uint32_t)c;
                };
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const uint4 v = tr[q];
                    if (2 * q < NTH) tcur[2 * q] = coarse(v.x, v.y);
                    if (2 * q + 1 < NTH) tcur[2 * q + 1] = coarse(v.z, v.w);
                }
            }
            // one rollout step; returns true when the rollout must stop after it
            // LEANH: `h` holds the step count BEHIND the trip, two more than before its first step, one add per trip; step "a"
            // (second_tag false) is step h - 2 and stops at the limit if h - 1 >= hmax, step "b" is step h - 1 and stops if
            // h >= hmax.  The loop below leaves h as the number of steps made, as the other forms do.
            auto step = [&](auto second_tag, double &r_mine, double &g_mine, const double r_prev, const double g_prev, bool add_prev,
                            const RollGen &gcur, RollGen &gspec, uint64_t &unext) -> bool {
                constexpr int SECOND = decltype(second_tag)::value ? 1 : 0;
                // searchsorted(cdf, u, 'right') = #{a : cdf[a] <= u} = #{a : thr[a] <= k}
                int act = 0;
                if constexpr (ATAB) {
                    act = (int)act_next;
                } else
                if (SP) {
                    // thr <= k is decided by the top bits unless they are equal: th < kh => thr < (th+1) << shift
                    // <= k;  th > kh => thr >= th << shift > k (also for the saturated th of thr = 2^53)
                    const uint32_t kh = (uint32_t)(u >> p.pol_shift);
                    bool ambiguous = false;
#pragma unroll
                    for (int a = 0; a < NTH; ++a) {
                        act += tcur[a] < kh ? 1 : 0;
                        ambiguous |= tcur[a] == kh;
                    }
                    if (ambiguous) {
                        const uint64_t *tx = p.pol_thr + (long)s * p.pol_stride;
                        act = 0;
#pragma unroll
                        for (int a = 0; a < NTH; ++a) act += tx[a] <= u ? 1 : 0;
                    }
                } else if (AT > 0) {
                    // (the last threshold, 2^53, is never reached; thresholds of 2^53 before it -- trailing zero
                    // probabilities -- are ~0 here and form a suffix: thr_valid caps the count so that even the draw
                    // 2^64 - 1 selects what searchsorted selects)
#pragma unroll
                    for (int a = 0; a < NTH; ++a) act += p.thr_arg[a] <= u ? 1 : 0; // scalar operands
                    act = min(act, p.thr_valid);
                } else {
                    for (int a = 0; a < A; ++a) act += thr[a] <= u ? 1 : 0;
                }
                g_mine = LEANH ? gpow[h - 2 + SECOND] : gpow[h];
                // 32-bit record index (S * |A| < 2^31): one multiply-add instead of a 64-bit address chain; a 24-bit one where the
                // form bounds S * |A| below 2^24 (the LDS-resident model: three bytes per (s, a) in at most 160 KB)
                const unsigned ridx = PCGW && LDSR ? __umul24((unsigned)s, (unsigned)A) + (unsigned)act : (unsigned)(s * A + act);
                bool term_h;
                if (CART) {
                    gspec = gcur;
                    unext = gspec.next64() >> USH;
                    term_h = cartpole_step(p.cp, x4, act, p.cp_sincos, sctab);
                    total += g_mine * 1.0;
                } else if (LDSR) {
                    const unsigned idx = ridx;
                    uint32_t e = t16[idx];
                    // LEANI: the word as the load leaves it, 32 bits with the upper half clear.  (What the compiler sees as a
                    // 16-bit value it masks in 16 bits and then extends for the index: an `and` with 0xffff behind the `and` with
                    // 0x7fff.  No instruction here.)
                    if constexpr (LEANI) asm("" : "+v"(e));
                    r_mine = rdict[r8[idx]];
                    gspec = gcur;
                    unext = gspec.next64() >> USH;
                    if constexpr (ATAB) act_next = table_action(unext);
                    // (the first step of a rollout has no previous reward: r_prev = g_prev = 0.0 then, and adding +0.0 changes no bit
                    // of a return that is never -0 -- no select on `add_prev`)
                    total += g_prev * r_prev;
                    // (LEANI: the word is below 2^16, so bit 15 is one unsigned compare; a test of the bit is an `and` and a compare)
                    const bool next_term = LEANI ? e > 0x7fffu : (e & 0x8000u) != 0;
                    if constexpr (TERMTAB) {
                        term_h = next_term;
                    } else {
                        term_h = p.done_on_next ? next_term : cur_term;
                        cur_term = next_term;
                    }
                    s = (int32_t)(e & 0x7fffu);
                } else if (SP && NTH <= 4 && p.pol_packed) {
                    // one 16-byte record: the 10 top bits of each threshold ride in the spare bits of next / flags
                    // (an ambiguous draw -- ~0.4 % of the steps -- fetches the exact row, as above)
                    const uint4 q0 = p.pol_frec[ridx];
                    gspec = gcur;
                    unext = gspec.next64() >> USH; // overlaps the gather
                    term_h = (q0.y & done_bit) != 0;
                    s = (int32_t)(q0.x & 0xfffffu);
                    total += g_mine * __hiloint2double((int)q0.w, (int)q0.z);
                    tcur[0] = (q0.x >> 20) & 1023u;
                    if (NTH > 1) tcur[NTH > 1 ? 1 : 0] = (q0.y >> 2) & 1023u;
                    if (NTH > 2) tcur[NTH > 2 ? 2 : 0] = (q0.y >> 12) & 1023u;
                    if (NTH > 3) tcur[NTH > 3 ? 3 : 0] = (q0.y >> 22) & 1023u;
                } else if (SP) {
                    const uint4 *fr = p.pol_frec_roll + (size_t)ridx * (1 + NQ32);
                    const uint4 q0 = fr[0];
                    uint4 qt[NQ32];
#pragma unroll
                    for (int q = 0; q < NQ32; ++q) qt[q] = fr[1 + q];
                    gspec = gcur;
                    unext = gspec.next64() >> USH; // overlaps the gather
                    term_h = (q0.y & done_bit) != 0;
                    s = (int32_t)q0.x;
                    total += g_mine * __hiloint2double((int)q0.w, (int)q0.z);
#pragma unroll
                    for (int q = 0; q < NQ32; ++q) {
                        if (4 * q < NTH) tcur[4 * q] = qt[q].x;
                        if (4 * q + 1 < NTH) tcur[4 * q + 1] = qt[q].y;
                        if (4 * q + 2 < NTH) tcur[4 * q + 2] = qt[q].z;
                        if (4 * q + 3 < NTH) tcur[4 * q + 3] = qt[q].w;
                    }
                } else {
                    const Rec rc = rec[ridx];
                    gspec = gcur;
                    unext = gspec.next64() >> USH; // overlaps the gather
                    term_h = (rc.flags & done_bit) != 0;
                    s = rc.next;
                    total += g_mine * rc.reward;
                }
                // (st and steps_taken advance with h: added once after the rollout; the env's step limit is folded into hmax --
                // three vector instructions fewer in a step that issues ~50)
#ifdef MP_PROFILE
                ++n_roll;
#endif
                if constexpr (LEANH) {
                    return term_h || (SECOND ? h >= hmax : h > hmax);
                } else {
                    ++h;
                    return term_h || h >= hmax;
                }
            };
            while (true) {
                uint64_t un;
                if constexpr (LEANH) h += 2;
                if (step(std::false_type{}, r_a, g_a, r_b, g_b, have_b, ga, gb, un)) { stopped_in_a = true; break; }
                u = un;
                have_b = true;
                if (step(std::true_type{}, r_b, g_b, r_a, g_a, true, gb, ga, un)) { stopped_in_a = false; break; }
                u = un;
            }
            if constexpr (LEANH) h -= stopped_in_a ? 1 : 0;
            if (LDSR) total += stopped_in_a ? g_a * r_a : g_b * r_b;
            roll_gen_commit(g, stopped_in_a ? ga : gb); // the generator whose draw was consumed last
            st += h - depth; steps_taken += h - depth;
        }
        if constexpr (TREE_PRIO > 0) __builtin_amdgcn_s_setprio(TREE_PRIO);
        PROF_T(c3);
        // ---- backup, mcts.py:248-265: the same return for every node on the path
        auto inv_fast = [&](int c) { if constexpr (RC) return inv_tab(c); else return inv(c); };
        // the new statistics of a path node below the root's children: value and count as ONE 12-byte store, first_child left alone
        // -- but the LEAF (leaf1: the first node a backup writes) whole, with the first_child the expansion gave it (`fc`; that of
        // the descent's last read where nothing expanded)
        typedef uint32_t stat3 __attribute__((ext_vector_type(3), may_alias));
        auto put_stats = [&](int n, double v, int cnt, bool leaf) {
            if (LEAF1 && leaf) {
                UctNode w;
                w.value = v; w.count = cnt; w.first_child = fc;
                tree.at(n) = w;
            } else {
                stat3 w;
                w.x = (uint32_t)__double2loint(v); w.y = (uint32_t)__double2hiint(v); w.z = (uint32_t)cnt;
                *reinterpret_cast<stat3 *>(&tree.at(n)) = w;
            }
        };
        bool leaf = leaf1; // (uniform over the lanes of a trip: every lane's first)
        if (RC && beyond) {
            // a count of this wave may lie beyond the tables: every level of the path, the root and its child included, through
            // ONE body with the division in it (the values and the order of operations of the table form below)
            for (int d = depth; d >= 0; --d) {
                int n = 0;
                if (d >= 1) PATH_GET(n, d);
                const int a1 = n - tree.handle(1, 0); // d == 1: which child of the root
                double v = tv0;
                int cnt = tc0;
                if (d >= 2 + KEEP) {
                    const UctNode c = tree.at(n);
                    v = c.value; cnt = c.count;
                } else {
#pragma unroll
                    for (int a = 0; a < AR; ++a) { v = (d == 1 && a1 == a) ? tv[a] : v; cnt = (d == 1 && a1 == a) ? tc[a] : cnt; }
#pragma unroll
                    for (int i = 0; i < KEEP; ++i) { v = d == 2 + i ? kv[i] : v; cnt = d == 2 + i ? kc[i] : cnt; }
                }
                cnt += 1;
                v += inv(cnt) * (total - v);
                if (d >= 2) {
                    put_stats(n, v, cnt, leaf);
                } else if (d == 1) {
#pragma unroll
                    for (int a = 0; a < AR; ++a) { tv[a] = a1 == a ? v : tv[a]; tc[a] = a1 == a ? cnt : tc[a]; }
                } else {
                    tv0 = v; tc0 = cnt;
                }
                leaf = false;
            }
        } else {
            for (int d = depth; d >= (RC ? 2 : 0); --d) {
                int n;
                PATH_GET(n, d);
                if (RC && d < 2 + KEEP) {
                    double v = kv[0];
                    int cnt = kc[0];
#pragma unroll
                    for (int i = 1; i < KEEP; ++i) { v = d == 2 + i ? kv[i] : v; cnt = d == 2 + i ? kc[i] : cnt; }
                    cnt += 1;
                    v += inv_fast(cnt) * (total - v);
                    put_stats(n, v, cnt, leaf);
                } else {
                    UctNode c = tree.at(n);
                    c.count += 1;
                    c.value += inv_fast(c.count) * (total - c.value);
                    if constexpr (RC) {
                        put_stats(n, c.value, c.count, leaf);
                    } else {
                        tree.at(n).value = c.value;
                        tree.at(n).count = c.count;
                    }
                }
                leaf = false;
            }
            if (RC) {
                if (depth >= 1) {
                    int n;
                    PATH_GET(n, 1);
                    n -= tree.handle(1, 0); // level-1 node: which child of the root
                    double v = tv[0];
                    int cnt = tc[0];
#pragma unroll
                    for (int a = 1; a < AR; ++a) { v = n == a ? tv[a] : v; cnt = n == a ? tc[a] : cnt; }
                    cnt += 1;
                    v += inv_fast(cnt) * (total - v);
#pragma unroll
                    for (int a = 0; a < AR; ++a) { tv[a] = n == a ? v : tv[a]; tc[a] = n == a ? cnt : tc[a]; }
                }
                tc0 += 1;
                tv0 += inv_fast(tc0) * (total - tv0);
            }
        }
#ifdef MP_PROFILE
        { const long long c4 = clock64(); t_sel += c1 - c0; t_expd += c2 - c1; t_roll += c3 - c2; t_bak += c4 - c3; }
#endif
    }
    if constexpr (BAL) {
        // done planning: nobody's mate any more (what follows -- the root's write-back and the plan's read-out -- is short)
        if ((((uint32_t)r) & 63u) == 0u) bal_store(&lds_bal[((uint32_t)r >> 6) & (kUctBalWords - 1)], kUctBalGone);
    }
    WAVE_STAMP(2);
    if constexpr (TREE_PRIO > 0) __builtin_amdgcn_s_setprio(0);
#ifdef MP_PROFILE
    if (r == 0)
        printf("uct prof wave0: total=%lld select=%lld expand=%lld rollout=%lld backup=%lld | lane0 select steps=%lld rollout steps=%lld\n",
               (long long)(clock64() - t_all0), t_sel, t_expd, t_roll, t_bak, n_sel, n_roll);
#endif
    if (!owner) return;                      // (QD: the helper lanes held no tree)
    if (CART && (lane & ((1 << p.rep_shift) - 1)) != 0) return;   // (replicas of a CartPole root: the first lane reports)
    // READ-OUT FROM REGISTERS (profiles/uct_step_fixed_costs.md).  The last wave of every SIMD runs what follows alone, every
    // round trip to memory exposed at the end of the launch.  With the root and its children in registers (RC, tf0 == 1) the root's
    // word, level 0 of the plan's walk and the root's statistics are taken from them -- no load of what the lines above have just
    // stored -- and every level below loads each stored child once, picks by selects and stores its action last: one round trip
    // per level (read-out 20.5 -> 10.2 us per wave, headline step 0.548 -> 0.536 ms).  A re-rooted tree whose root's children
    // are not at id 1 and the generic |A| keep the loads; so does the four-lane form of |A| >= 7, which spills already and would
    // spill four VGPRs more (|A| = 7: 8 bytes of scratch, |A| = 8: 4).  -DMP_UCT_READOUT_REGS=0: everything loaded back, for A/B runs.
    constexpr bool RREG = RC && MP_UCT_READOUT_REGS != 0 && !(QD && AT >= 7);
    int root_word = -1; // RREG: first_child of the root as stored (VMASK: with the full mask)
    if (RC) {
        UctNode w;
        w.value = tv0; w.count = tc0; w.first_child = tf0;
        if (VMASK && tf0 >= 0) w.first_child = tf0 | (((1 << AR) - 1) << kUctMaskShift); // (all its children are stored below)
        root_word = w.first_child;
        tree[0] = w;
        if (tf0 == 1) {
#pragma unroll
            for (int a = 0; a < AR; ++a) {
                w.value = tv[a]; w.count = tc[a]; w.first_child = tf[a];
                tree.child(1, a) = w;
            }
        }
    }
    g.store(p.rng + (long)r * 6);
    const bool root_regs = RREG && tf0 == 1; // the root's children are tv[] / tc[] / tf[]
    // ---- AbstractPlanner.get_plan (abstract.py:143-156) with MCTSNode.selection_rule
    // (mcts.py:212-218): most visited child, ties -> first maximal value among them
    {
        int len = 0;
        int fc = RREG ? root_word : tree[0].first_child;
        int at_c = 0; // VDEFER: the count of the node whose children are read (the root's group is always stored)
        int32_t *const plan = p.plans ? p.plans + (long)r * p.max_plan_len : nullptr;
        if (root_regs) {
            // level 0: the root's children, registers
            int mc = tc[0];
#pragma unroll
            for (int a = 1; a < AR; ++a) mc = max(mc, tc[a]);
            int best = -1, bfc = -1, bc = 0;
            double bv = 0.0;
#pragma unroll
            for (int a = 0; a < AR; ++a) {
                const bool take = tc[a] == mc && (best < 0 || tv[a] > bv);
                best = take ? a : best; bv = take ? tv[a] : bv; bfc = take ? tf[a] : bfc; bc = take ? tc[a] : bc;
            }
            if (plan && len < p.max_plan_len) plan[len] = best;
            ++len;
            at_c = bc;
            fc = bfc;
        }
        while (fc >= 0) {
            if (VDEFER && vdefer && at_c == 1) {
                // a group that was never stored, all {0.0, 0, -1}: the first action, whose node has no children
                if (plan && len < p.max_plan_len) plan[len] = 0;
                ++len;
                break;
            }
            // VMASK: a child whose bit in the word is clear was never stored, the constant node
            unsigned stored = ~0u;
            if (VMASK) { stored = (unsigned)fc >> kUctMaskShift; fc &= kUctChildBits; }
            if constexpr (RREG) {
                // one level: every stored child loaded once, the pick and what the walk needs of it by selects, then the store
                UctNode *grp = &tree.child(fc, 0);
                UctNode c[AR];
#pragma unroll
                for (int a = 0; a < AR; ++a) {
                    c[a].value = 0.0; c[a].count = 0; c[a].first_child = -1;
                    if (!VMASK || ((stored >> a) & 1u)) c[a] = tree.sibling(grp, a);
                }
                int mc = c[0].count;
#pragma unroll
                for (int a = 1; a < AR; ++a) mc = max(mc, c[a].count);
                int best = -1, bfc = -1, bc = 0;
                double bv = 0.0;
#pragma unroll
                for (int a = 0; a < AR; ++a) {
                    const bool take = c[a].count == mc && (best < 0 || c[a].value > bv);
                    best = take ? a : best; bv = take ? c[a].value : bv; bfc = take ? c[a].first_child : bfc; bc = take ? c[a].count : bc;
                }
                if (plan && len < p.max_plan_len) plan[len] = best;
                ++len;
                at_c = bc;
                fc = bfc;
            } else {
                auto child = [&](int a) {
                    UctNode c;
                    c.value = 0.0; c.count = 0; c.first_child = -1;
                    if (!VMASK || ((stored >> a) & 1u)) c = tree.child(fc, a);
                    return c;
                };
                int mc = child(0).count;
                for (int a = 1; a < A; ++a) mc = max(mc, child(a).count);
                int best = -1;
                double bv = 0.0;
                for (int a = 0; a < A; ++a) {
                    const UctNode c = child(a);
                    if (c.count == mc && (best < 0 || c.value > bv)) { best = a; bv = c.value; }
                }
                if (plan && len < p.max_plan_len) plan[len] = best;
                ++len;
                const UctNode b = child(best);
                at_c = b.count;
                fc = b.first_child;
            }
        }
        if (plan)
            for (int i = len; i < p.max_plan_len; ++i) plan[i] = -1;
        if (p.plan_len) p.plan_len[r] = len;
    }
    if (p.n_nodes_out) p.n_nodes_out[r] = n_nodes;
    if (p.root_value) p.root_value[r] = RREG ? tv0 : tree[0].value;
    if (p.env_steps) p.env_steps[r] = (int64_t)steps_taken;
    if (root_regs || (RREG && tf0 < 0)) {
        // the root's children from registers; a root that never expanded has none
#pragma unroll
        for (int a = 0; a < AR; ++a) {
            if (p.root_child_count) p.root_child_count[(long)r * A + a] = tf0 < 0 ? 0 : max(tc[a], 0);
            if (p.root_child_value) p.root_child_value[(long)r * A + a] = tf0 < 0 ? 0.0 : tv[a];
        }
    } else {
        int rfc = RREG ? tf0 : tree[0].first_child;
        if (VMASK) rfc = uct_word_child(rfc); // (the root's children are all stored)
        for (int a = 0; a < A; ++a) {
            if (p.root_child_count) p.root_child_count[(long)r * A + a] = rfc >= 0 ? max(tree.child(rfc, a).count, 0) : 0;
            if (p.root_child_value) p.root_child_value[(long)r * A + a] = rfc >= 0 ? tree.child(rfc, a).value : 0.0;
        }
    }
    WAVE_STAMP(3);
#undef WAVE_STAMP
}

// ---- ONE ROOT PER WORKGROUP (round 5): the plan of a single agent's act(), and of every batch small enough to give each root
// a CU of its own.  A lone root is one dependency chain; uct_kernel runs it in one lane of a wave, the tree in global memory
// (a dependent L2 round trip per scored level and per backed-up node), every rollout step behind numpy's 128-bit generator
// step.  Here the whole WAVEFRONT works for the root:
//   * the model (3 B per (s, a)), the per-call tables AND THE TREE live in LDS (a 33-episode tree is 2.7 KB); sixteen waves
//     stage them, one stays;
//   * a level's |A| children are scored by |A| lanes, a path's nodes are backed up by as many lanes at once;
//   * a rollout's actions do not depend on the states it visits (state-independent policy): lane l draws action l from the
//     generator l + 1 steps ahead (one table-driven jump: A^(l+1) s + inc G_(l+1)), then the walk is H dependent LDS reads
//     and nothing else -- the rewards are looked up by the lanes in parallel afterwards and added in the reference's order;
//     the generator then jumps by the n draws the walk consumed, so the stream stays the reference's.
// Same trees, plans, statistics and generator records as uct_kernel (every single-root golden runs through it when forced:
// MP_UCT_LONE=1); the tree is written to global memory in the group-interleaved layout at the end (export, re-rooting).
// EACH (round 6): ONE MDP PER ROOT -- a batch model (mp_model_load_table_batch: the finite MDPs of a batch of episodes, each
// extracted from its own environment) where root r plans on MDP root_state[r] / Sb.  The union model is too large for the compact
// LDS forms (S = NB * Sb >= 32 768 states), but a root only ever visits ITS MDP: the workgroup stages that MDP's Sb * |A| records
// from the 16-byte global records into LDS as {uint16 local next state | bit 15 terminal[next]} + the reward itself (f64: no
// reward dictionary, any number of distinct rewards) -- 10 B per (s, a), 6 KB for a 120-state highway grid -- and everything
// else is the lone-root kernel: tree in LDS, a level scored across lanes, the rollout's draws by jump-ahead in the lanes.  One
// wave per workgroup (small MDPs) so that 4096 roots are 4096 wavefronts, four per SIMD.
// MW (round 6): SEVERAL ROOTS PER WORKGROUP, A WAVEFRONT EACH, around ONE copy of a model that fills the LDS -- the headline table's
// transitions are 100 of the CU's 160 KB, so with the reward indices beside them only one root fits a CU (256 roots per launch).
// Here the workgroup keeps the transitions only, p.waves (2 / 4 / 8) planning wavefronts stay after the staging, each with its own
// tree and its own copy of the jump table behind them, one or two per SIMD; an episode's rewards come from the model's 16-byte
// records in L2 (ONE vector load for the whole episode: lane l its step's reward) instead of the two LDS round trips.
template <int AT, bool EACH = false, bool MW = false>
__global__ __launch_bounds__(EACH ? 256 : 1024, EACH ? 4 : 1) void uct_lone_kernel(UctArgs p)
{
    static_assert(!(EACH && MW), "one MDP per root is staged per workgroup: one root each");
    static_assert(AT >= 2 && AT <= 8, "|A| with a compile-time specialisation");
    constexpr int A = AT, NTH = AT - 1;
    extern __shared__ __attribute__((aligned(16))) double lds_d[];
    const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
    const int H = p.horizon, E = p.episodes, TE = p.table_n;
    double *gpow = lds_d;                   // [H + 1]  gamma ** h
    double *tp = gpow + (H + 1) + A;        // [A]      temperature * |A| * prior[a]
    double *rcp = tp + A;                   // [TE + 1]  1.0 / n
    double *tpdiv = rcp + (TE + 1);         // [A][TE+2] temperature * |A| * prior[a] / n
    const int ntab = (H + 1) + 2 * A + (TE + 1) + A * (TE + 2);
    const int ntab2 = (ntab + 1) & ~1;
    const int SA = (EACH ? p.Sb : p.S) * A;                                       // (s, a) pairs of the model this root plans on
    const double *rdict = lds_d + ntab2;                                          // shared model: [n_rdict] distinct rewards (not MW)
    double *rew = lds_d + ntab2;                                                  // EACH: [SA] the rewards themselves
    uint16_t *t16 = EACH ? reinterpret_cast<uint16_t *>(rew + ((SA + 1) & ~1))
                         : reinterpret_cast<uint16_t *>(lds_d + ntab2 + (MW ? 0 : ((p.n_rdict + 1) & ~1)));
    uint8_t *r8 = reinterpret_cast<uint8_t *>(t16 + ((SA + 7) & ~7));             // shared model: [SA] reward indices (not MW)
    // per planning wavefront: its copy of the jump table [H + 5][8] (it gets the root's inc G_j), its tree [cap] and a node's
    // exploration term at its count [cap]
    uint32_t *jump0 = (EACH || MW) ? reinterpret_cast<uint32_t *>(r8) : reinterpret_cast<uint32_t *>(r8 + ((SA + 15) & ~15));
    const int W = MW ? p.waves : 1;
    const int wstride = ((H + 5) * 8 + p.cap * 6 + 3) & ~3;                       // 32-bit words per wavefront (16-byte multiples)
    uint32_t *jump = jump0 + (MW ? (tid >> 6 < W ? tid >> 6 : 0) * wstride : 0);
    UctNode *tnode = reinterpret_cast<UctNode *>(jump + (H + 5) * 8);            // [cap]
    double *texpl = reinterpret_cast<double *>(tnode + p.cap);                   // [cap]
    // (the [H + 1] words behind texpl held the path until round 6: it now lives in a register, one node per lane)
    int r = blockIdx.x;
    int32_t s0g = MW ? 0 : __builtin_amdgcn_readfirstlane(p.root_state[r]);      // (global state of a batch model)
    const int32_t sbase = EACH ? (s0g / p.Sb) * p.Sb : 0;                         // first global state of this root's MDP
    for (int w = 0; w < W; ++w)
        for (int i = tid; i < (H + 5) * 8; i += nthreads) jump0[w * wstride + i] = p.jump[i];
    for (int i = tid; i < ntab; i += nthreads) lds_d[i] = p.tab[i];
    if constexpr (EACH) {
        const Rec *src = p.rec + (long)sbase * A;
        for (int i = tid; i < SA; i += nthreads) {
            const Rec rc = src[i];
            t16[i] = (uint16_t)((uint32_t)(rc.next - sbase) | ((rc.flags & 2u) ? 0x8000u : 0u));
            rew[i] = rc.reward;
        }
    } else {
        if constexpr (!MW) {
            for (int i = tid; i < p.n_rdict; i += nthreads) lds_d[ntab2 + i] = p.rdict[i];
            const int n16 = (p.S * A + 15) >> 4; // (the device arrays are padded to whole 16-byte chunks)
            const uint4 *src = reinterpret_cast<const uint4 *>(p.r8);
            uint4 *dst = reinterpret_cast<uint4 *>(r8);
            for (int i = tid; i < n16; i += nthreads) dst[i] = src[i];
        }
        const int n = p.S * A, n8 = n >> 3;
        const uint4 *src2 = reinterpret_cast<const uint4 *>(p.t16);
        uint4 *dst2 = reinterpret_cast<uint4 *>(t16);
        for (int i = tid; i < n8; i += nthreads) dst2[i] = src2[i];
        for (int i = (n8 << 3) + tid; i < n; i += nthreads) t16[i] = p.t16[i];
    }
    __syncthreads();
    if (tid >= 64 * W) return; // (the staging waves are done; no barrier below)
    if constexpr (MW) {
        r = blockIdx.x * W + (tid >> 6);
        if (r >= p.n_roots) return;
        s0g = __builtin_amdgcn_readfirstlane(p.root_state[r]);
    }
    // MCTSNode.selection_strategy's exploration term temperature |A| prior[a] / (count + 1) (mcts.py:275-286): from the host's
    // quotient table, or the same IEEE division beyond it.  Kept PER NODE beside the tree and refreshed by the backup (which
    // changes the count), so that scoring a level is one LDS round trip, not two
    auto explore = [&](int a, int cnt1) { return cnt1 <= TE + 1 ? tpdiv[a * (TE + 2) + cnt1] : tp[a] / (double)cnt1; };
    auto inv = [&](int c) { return c <= TE ? rcp[c] : 1.0 / (double)c; };
    Pcg64U g;                                    // (one generator for the wave, in scalar registers)
    g.load(p.rng + (long)r * 6);
    const int32_t s0 = s0g - sbase;                                    // (local to the staged MDP)
    const int32_t st0 = p.root_steps ? __builtin_amdgcn_readfirstlane(p.root_steps[r]) : 0;
    const bool root_term = (p.rec[(long)s0g * A].flags & 1u) != 0; // terminal flag of the root state itself ("source" rule)
    int n_nodes = 1, steps_taken = 0;
    if (lane == 0) { UctNode n; n.value = 0.0; n.count = 0; n.first_child = -1; tnode[0] = n; texpl[0] = 0.0; } // mcts.py:129-130 reset()
    // A jump by j steps is state <- A^j state + inc G_j; the increment is the root's for the whole plan, so this workgroup's copy of
    // the jump table gets inc G_j in place of G_j once (lane l: j = l + 1; the draws use j <= H <= 63) -- every rollout's draw is then
    // ONE 128-bit product per lane, not two
    if (lane < H) {
        const int j = lane + 1;
        uint32_t gn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) gn[i] = jump[j * 8 + 4 + i];
        uint64_t lo, hi;
        Pcg64::mul128v(g.inc_lo, g.inc_hi, gn, lo, hi);
        jump[j * 8 + 4] = (uint32_t)lo; jump[j * 8 + 5] = (uint32_t)(lo >> 32);
        jump[j * 8 + 6] = (uint32_t)hi; jump[j * 8 + 7] = (uint32_t)(hi >> 32);
    }
    __builtin_amdgcn_wave_barrier();
    const int la = lane < A ? lane : 0;
    const double expl1 = explore(la, 1);          // a fresh child's term (count 0)
    // (round 6, second pass) An env step's reward comes through two more LDS reads (reward index -> reward) that the state chain
    // does not need.  A lone wave issues an instruction every ~5 cycles whatever it depends on, so what a step costs is its
    // instruction COUNT: the steps of an episode (descent and rollout alike) only note their (s, a) index in lane `depth` of one
    // register; after the walk the lanes look up their steps' rewards AT ONCE (two LDS reads for the whole episode), multiply by
    // gamma ** lane, and the products are added one by one in the reference's order (mcts.py:160-177: total += gamma ** h * r).
    // The three-stage reward pipeline this replaces cost ~25 of a rollout step's 43 instructions.
    const double gpl = gpow[min(lane, H)];        // gamma ** lane
    int idxv = 0;                                 // lane l: s * |A| + a of the episode's step l (stale beyond: valid, unused)
    uint32_t sv = 0;                              // lane l: the state the rollout's step at depth l leaves from (noted by the walk)
    int pathv = 0;                                // lane l: the tree node at depth l of the episode's path (lane 0: the root)
    const uint32_t tshift = p.done_on_next ? 0u : 16u;
    const uint32_t t16_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t *)t16; // byte offset of t16 in LDS
#ifdef MP_PROFILE
    long long pt[6] = {0, 0, 0, 0, 0, 0}, pn_sel = 0, pn_roll = 0;
    const long long pt_all = clock64();
#define MP_LT(i_) do { const long long c_ = clock64(); pt[i_] += c_ - pc; pc = c_; } while (0)
#else
#define MP_LT(i_) do { } while (0)
#endif
    for (int ep = 0; ep < E; ++ep) { // mcts.py:179-184
#ifdef MP_PROFILE
        long long pc = clock64();
#endif
        int32_t s = s0, st = st0;
        int node = 0, depth = 0, n_roll = 0;
        bool terminal = false;
        // the records of the last two steps, the newer in the low half: bit 15 of the one the terminal rule names ends the descent
        // ("next" rule: the step just taken; "source" rule: the one before, i.e. the state the step left from was terminal)
        uint32_t hist = root_term ? 0x8000u : 0u;
        int fc = __builtin_amdgcn_readfirstlane(tnode[0].first_child);
        // ---- selection, mcts.py:143-149: a level's children one per lane
        while (depth < H && fc >= 0 && !terminal) {
            const UctNode c = tnode[fc + la];
            const double ex = texpl[fc + la];
            // (every child's transition is read with the children, one per lane: the step of the picked one is then a readlane,
            // not a second LDS round trip behind the pick)
            const uint32_t cand = t16[s * A + la];
            const double sc = c.value + ex;
            // Node.random_argmax, abstract.py:296-311: the maxima = the children no other child beats (|A| independent compares
            // against the scores read off their lanes; a chain of maxima would be |A| dependent selects)
            unsigned long long ties = (1ull << A) - 1ull;
#pragma unroll
            for (int a = 0; a < A; ++a) ties &= ballot64(sc >= bcast_lane(sc, a));
            const int nt = __popcll(ties);
            int pick = nt > 1 ? (int)g.below((uint32_t)nt) : 0;
            pick = __builtin_amdgcn_readfirstlane(pick);
            unsigned long long t = ties;
            while (pick-- > 0) t &= t - 1;
            const int act = __ffsll((long long)t) - 1;
            const int nfc = __builtin_amdgcn_readlane(c.first_child, act);
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)cand, act);
            idxv = lane == depth ? s * A + act : idxv;
            hist = (hist << 16) | e;
            terminal = ((hist >> tshift) & 0x8000u) != 0;
            s = (int32_t)(e & 0x7fffu);
            ++st; ++steps_taken;
            node = fc + act;
            ++depth;
            pathv = lane == depth ? node : pathv;
            fc = nfc;
        }
        const bool cur_term = (hist & 0x8000u) != 0;
#ifdef MP_PROFILE
        pn_sel += depth;
#endif
        MP_LT(0);
        // ---- expansion, mcts.py:151-154 / 237-246
        if (fc < 0 && depth < H && (!terminal || node == 0)) {
            if (lane == 0) tnode[node].first_child = n_nodes;
            if (lane < A) {
                UctNode n;
                n.value = 0.0; n.count = 0; n.first_child = -1;
                tnode[n_nodes + lane] = n;
                texpl[n_nodes + lane] = expl1;
            }
            n_nodes += A;
        }
        MP_LT(1);
        // ---- rollout, mcts.py:156-157 / 160-177
        if (!terminal && depth < H) {
            // Lane h holds what the step at depth h needs: its action (lane h draws action h - depth of the rollout, from the
            // generator h - depth + 1 steps ahead) and, noted by the walk, the state it leaves from -- so the lanes form their
            // steps' (s, a) indices themselves afterwards.
            uint32_t act_l;
            Pcg64 q;                               // (the lanes' jumps: vector arithmetic on copies)
            q.s_hi = g.s_hi; q.s_lo = g.s_lo; q.inc_hi = g.inc_hi; q.inc_lo = g.inc_lo; q.has_uint32 = 0; q.uinteger = 0;
            {
                const int j1 = min(max(lane - depth + 1, 1), H); // (draws beyond the horizon / of the descent's lanes are never used)
                uint32_t an[4], ig[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { an[i] = jump[j1 * 8 + i]; ig[i] = jump[j1 * 8 + 4 + i]; }
                uint64_t p_lo, p_hi;                // A^j state + inc G_j, the second product from this root's table
                Pcg64::mul128v(q.s_lo, q.s_hi, an, p_lo, p_hi);
                const uint64_t q_lo = (uint64_t)ig[0] | ((uint64_t)ig[1] << 32), q_hi = (uint64_t)ig[2] | ((uint64_t)ig[3] << 32);
                const uint64_t lo = p_lo + q_lo;
                q.s_hi = p_hi + q_hi + (lo < p_lo ? 1ULL : 0ULL);
                q.s_lo = lo;
                const uint64_t u = q.output();     // searchsorted(cdf, u, 'right') on the raw 64-bit output
                int act = 0;
#pragma unroll
                for (int a = 0; a < NTH; ++a) act += p.thr_arg[a] <= u ? 1 : 0;
                act_l = (uint32_t)min(act, p.thr_valid);
            }
            MP_LT(2);
            // the walk: at most n_lim steps (horizon, the env's step limit).  The chain of a step is ONE multiply-add (LDS byte
            // address of the record = state * 2|A| + (2 a + the table's offset), the second term a scalar read off the action's lane)
            // and the read itself; the scalar side only tests the terminal bit and counts.
            int n_lim = H - depth;
            if (p.max_steps > 0 && p.max_steps - st < n_lim) n_lim = p.max_steps - st;
            if (n_lim < 1) n_lim = 1; // (the first step is unconditional, as in the reference's loop)
            const uint32_t act2 = 2u * act_l + t16_lds;
            const int h_end = depth + n_lim;
            // The walk, written out (inline assembly: the compiler rotates any C form of it back into read -> wait -> test, and a
            // lone wave pays ~20 cycles for every branch, taken or not -- tools/lds_chain.hip: the bare chain v_and -> v_mad_u32_u24
            // (state * 2|A| + action term) -> ds_read_u16 is 64 cycles a step, with two exit tests beside it 122).
            //  * GROUPS OF FOUR steps without a branch: each slot issues the read of its step (speculative: any record's next state
            //    is a valid state, its lane's action a valid action; what a step not taken leaves behind is never used) and, under
            //    that read's latency, notes the state the step leaves from in its lane, fetches the next action term and shifts the
            //    previous record's terminal bit into a scalar; ONE test per group finds the step the rollout ends with (the first set
            //    bit: "next" rule = the records of the four steps, "source" rule = the records before them).  Groups run while four
            //    more steps are within the horizon / step limit;
            //  * the remaining (< 4) steps one by one, each with its two tests (the same slot otherwise).
            // The walk starts from a VIRTUAL record: the state before the first step, bit 15 = "that state is terminal" under the
            // "source" rule -- the first step is then an ordinary one (unconditional: the reference's loop tests after the step).
            // Wait states by hand (the hazard pass does not look inside): a VALU that reads an SGPR / VCC a VALU wrote comes at
            // least two instructions later.
            uint32_t v1 = (uint32_t)s | (!p.done_on_next && cur_term ? 0x8000u : 0u);
            int h = depth;                              // (v1 = the record of the step at depth h - 1; h <= H <= 63: a lane)
            uint32_t done = 0;
            if (h + 4 <= h_end) {
                uint32_t w1, w2, w3, w4, t, a2, e, acc = 0, tst, h4;
#define MP_LONE_SLOT(WP, WN)                                                                       \
    "v_and_b32 %[t], 0x7fff, " WP "\n\t"                                                          \
    "v_mad_u32_u24 %[t], %[t], %[mul], %[a2]\n\t"                                                  \
    "ds_read_u16 " WN ", %[t]\n\t"                                                                 \
    "v_cmp_eq_u32 vcc, %[h], %[lane]\n\t"                                                          \
    "v_readfirstlane_b32 %[e], " WP "\n\t"                                                         \
    "s_add_i32 %[h], %[h], 1\n\t"                                                                  \
    "v_cndmask_b32 %[sv], %[sv], " WP ", vcc\n\t"                                                  \
    "v_readlane_b32 %[a2], %[act2], %[h]\n\t"                                                      \
    "s_lshr_b32 %[e], %[e], 15\n\t"                                                                \
    "s_lshl1_add_u32 %[acc], %[acc], %[e]\n\t"                                                     \
    "s_waitcnt lgkmcnt(0)\n\t"
#define MP_LONE_GROUPS(TEST)                                                                       \
    asm volatile("s_nop 3\n\t"                                                                     \
                 "v_readlane_b32 %[a2], %[act2], %[h]\n\t"                                          \
                 "s_nop 1\n\t"                                                                      \
                 "1:\n\t"                                                                           \
                 MP_LONE_SLOT("%[v1]", "%[w1]") MP_LONE_SLOT("%[w1]", "%[w2]")                      \
                 MP_LONE_SLOT("%[w2]", "%[w3]") MP_LONE_SLOT("%[w3]", "%[w4]")                      \
                 TEST                                                                               \
                 "s_cbranch_scc1 2f\n\t"                                                            \
                 "v_mov_b32 %[v1], %[w4]\n\t"                                                       \
                 "s_add_i32 %[h4], %[h], 4\n\t"                                                     \
                 "s_cmp_le_u32 %[h4], %[hend]\n\t"                                                  \
                 "s_cbranch_scc1 1b\n\t"                                                            \
                 "s_mov_b32 %[done], 0\n\t"                                                         \
                 "s_branch 3f\n\t"                                                                  \
                 "2:\n\t"               /* the group's step tst names is the last: (leading zeros of tst) - 27 of its 4 were taken */ \
                 "s_flbit_i32_b32 %[tst], %[tst]\n\t"                                               \
                 "s_add_i32 %[h], %[h], %[tst]\n\t"                                                 \
                 "s_sub_i32 %[h], %[h], 31\n\t"                                                     \
                 "s_mov_b32 %[done], 1\n\t"                                                         \
                 "3:\n\t"                                                                           \
                 : [h] "+s"(h), [sv] "+v"(sv), [v1] "+v"(v1), [acc] "+s"(acc), [done] "+s"(done), [w1] "=&v"(w1), [w2] "=&v"(w2), \
                   [w3] "=&v"(w3), [w4] "=&v"(w4), [t] "=&v"(t), [a2] "=&s"(a2), [e] "=&s"(e), [tst] "=&s"(tst), [h4] "=&s"(h4)  \
                 : [act2] "v"(act2), [lane] "v"(lane), [hend] "s"(h_end), [mul] "n"(2 * A)          \
                 : "vcc", "scc", "memory")
                if (p.done_on_next)
                    MP_LONE_GROUPS("v_readfirstlane_b32 %[e], %[w4]\n\t"
                                   "s_lshr_b32 %[e], %[e], 15\n\t"
                                   "s_lshl1_add_u32 %[tst], %[acc], %[e]\n\t"
                                   "s_and_b32 %[tst], %[tst], 15\n\t");
                else
                    MP_LONE_GROUPS("s_and_b32 %[tst], %[acc], 15\n\t");
#undef MP_LONE_GROUPS
#undef MP_LONE_SLOT
            }
            done = (uint32_t)__builtin_amdgcn_readfirstlane((int)done);   // (scalar for the compiler too, whatever it made of the merge)
            h = __builtin_amdgcn_readfirstlane(h);
            if (!done) {
                uint32_t pe = 0;                        // (the record before v1; a set bit 15 would have ended the walk already)
                uint32_t v2, t, a2, e, h1;
#define MP_LONE_HALF(V1, V2, STOP)                                                                 \
    "v_and_b32 %[t], 0x7fff, " V1 "\n\t"                                                          \
    "v_mad_u32_u24 %[t], %[t], %[mul], %[a2]\n\t"                                                  \
    "ds_read_u16 " V2 ", %[t]\n\t"                                                                 \
    "v_cmp_eq_u32 vcc, %[h], %[lane]\n\t"                                                          \
    "v_readfirstlane_b32 %[e], " V1 "\n\t"                                                         \
    "s_add_i32 %[h1], %[h], 1\n\t"                                                                 \
    "v_cndmask_b32 %[sv], %[sv], " V1 ", vcc\n\t"                                                  \
    "v_readlane_b32 %[a2], %[act2], %[h1]\n\t"                                                     \
    STOP                                                                                           \
    "s_cbranch_scc1 2f\n\t"                                                                        \
    "s_cmp_ge_u32 %[h], %[hend]\n\t"                                                               \
    "s_cbranch_scc1 2f\n\t"                                                                        \
    "s_mov_b32 %[h], %[h1]\n\t"                                                                    \
    "s_waitcnt lgkmcnt(0)\n\t"
#define MP_LONE_WALK(STOP)                                                                         \
    asm volatile("s_nop 3\n\t"                                                                     \
                 "v_readlane_b32 %[a2], %[act2], %[h]\n\t"                                          \
                 "s_nop 1\n\t"                                                                      \
                 "1:\n\t" MP_LONE_HALF("%[v1]", "%[v2]", STOP) MP_LONE_HALF("%[v2]", "%[v1]", STOP)  \
                 "s_branch 1b\n\t"                                                                  \
                 "2:\n\t"                                                                           \
                 "s_waitcnt lgkmcnt(0)"                                                             \
                 : [h] "+s"(h), [sv] "+v"(sv), [v1] "+v"(v1), [pe] "+s"(pe), [v2] "=&v"(v2), [t] "=&v"(t), [a2] "=&s"(a2),       \
                   [e] "=&s"(e), [h1] "=&s"(h1)                                                     \
                 : [act2] "v"(act2), [lane] "v"(lane), [hend] "s"(h_end), [mul] "n"(2 * A)          \
                 : "vcc", "scc", "memory")
                if (p.done_on_next) MP_LONE_WALK("s_bitcmp1_b32 %[e], 15\n\t");
                else MP_LONE_WALK("s_bitcmp1_b32 %[pe], 15\n\ts_mov_b32 %[pe], %[e]\n\t");
#undef MP_LONE_WALK
#undef MP_LONE_HALF
            }
            MP_LT(3);
            const int n = h - depth;
            n_roll = n;
            st += n; steps_taken += n;
            idxv = lane >= depth ? (int)((sv & 0x7fffu) * A + act_l) : idxv;
            {   // the generator after the n draws the walk consumed = the state the lane of the last step jumped to for ITS draw
                const int src = h - 1;
                g.s_lo = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(q.s_lo >> 32), src) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)q.s_lo, src);
                g.s_hi = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(q.s_hi >> 32), src) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)q.s_hi, src);
            }
        }
        MP_LT(2);
        // the episode's return: its L steps' rewards looked up by L lanes, added in step order (a group of four per uniform test)
        double total = 0.0;
        {
            const int L = depth + n_roll;
            double rd;
            if constexpr (EACH) rd = rew[idxv]; else if constexpr (MW) rd = p.rec[idxv].reward; else rd = rdict[r8[idxv]];
            double prod = gpl * rd;
            prod = lane < L ? prod : 0.0;     // (+0.0 leaves a sum that started at +0.0 as it is, bit for bit)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (q * 4 >= L) break;
#pragma unroll
                for (int j = 0; j < 4; ++j) total += bcast_lane(prod, q * 4 + j);
            }
        }
#ifdef MP_PROFILE
        pn_roll += n_roll;
#endif
        MP_LT(4);
        // ---- backup, mcts.py:248-265: the same return for every node on the path, one node per lane
        __builtin_amdgcn_wave_barrier();
        if (lane <= depth) {
            const int nd = pathv;
            UctNode c = tnode[nd];
            c.count += 1;
            c.value += inv(c.count) * (total - c.value);
            tnode[nd].value = c.value;       // (first_child is left alone: the node may just have been expanded)
            tnode[nd].count = c.count;
            if (nd > 0) texpl[nd] = explore((nd - 1) % A, c.count + 1);
        }
        __builtin_amdgcn_wave_barrier();
        MP_LT(5);
    }
#undef MP_LT
#ifdef MP_PROFILE
    if (r == 0 && lane == 0)
        printf("uct_lone prof: total=%lld select=%lld expand=%lld draw+gen=%lld walk=%lld sum=%lld backup=%lld | levels=%lld rollout steps=%lld\n",
               (long long)(clock64() - pt_all), pt[0], pt[1], pt[2], pt[3], pt[4], pt[5], pn_sel, pn_roll);
#endif
    // the tree, to global memory in the group-interleaved layout (export, re-rooting by step_by_subtree)
    const TreeRef<2, AT> tree = tree_of<2, AT>(p.tree, r, p.cap, A);
    for (int i = lane; i < n_nodes; i += 64) tree[i] = tnode[i];
    if (lane == 0) {
        g.store(p.rng + (long)r * 6);
        // ---- AbstractPlanner.get_plan (abstract.py:143-156) with MCTSNode.selection_rule (mcts.py:212-218): most visited
        // child, ties -> first maximal value among them
        int len = 0;
        int fc = tnode[0].first_child;
        while (fc >= 0) {
            int mc = tnode[fc].count;
            for (int a = 1; a < A; ++a) mc = max(mc, tnode[fc + a].count);
            int best = -1;
            double bv = 0.0;
            for (int a = 0; a < A; ++a) {
                const UctNode c = tnode[fc + a];
                if (c.count == mc && (best < 0 || c.value > bv)) { best = a; bv = c.value; }
            }
            if (p.plans && len < p.max_plan_len) p.plans[(long)r * p.max_plan_len + len] = best;
            ++len;
            fc = tnode[fc + best].first_child;
        }
        if (p.plans)
            for (int i = len; i < p.max_plan_len; ++i) p.plans[(long)r * p.max_plan_len + i] = -1;
        if (p.plan_len) p.plan_len[r] = len;
        if (p.n_nodes_out) p.n_nodes_out[r] = n_nodes;
        if (p.root_value) p.root_value[r] = tnode[0].value;
        if (p.env_steps) p.env_steps[r] = (int64_t)steps_taken;
        const int rfc = tnode[0].first_child;
        for (int a = 0; a < A; ++a) {
            if (p.root_child_count) p.root_child_count[(long)r * A + a] = rfc >= 0 ? max(tnode[rfc + a].count, 0) : 0;
            if (p.root_child_value) p.root_child_value[(long)r * A + a] = rfc >= 0 ? tnode[rfc + a].value : 0.0;
        }
    }
}

// ---- FOUR ROOTS PER WAVEFRONT, ONE DPP ROW (16 LANES) EACH, ONE MDP PER ROOT (round 6): the batch of highway episodes, each with
// its own finite MDP (trainer/evaluation.py:139-194 x value_iteration.py:29-35).  uct_lone_kernel<.., EACH> gives such a root a
// whole wavefront; but a CDNA SIMD is 16 lanes wide -- a wave64 instruction holds it for 4 cycles whatever it computes -- so
// 4096 lone waves (4 per SIMD) run at a quarter of a lone wave's speed (measured: 0.176 ms, no better than one lane per root).
// Here a root gets exactly the 16 lanes it can use: |A| children scored by |A| lanes of ITS row, 16 rollout actions drawn at a
// time by jump-ahead (lane l of the row: the generator 16 k + l + 1 steps ahead), path nodes backed up one per lane; 4096 roots
// are 1024 wavefronts = one per SIMD, every instruction working for four roots.  Row-uniform values (state, depth, the
// generator) live in vector registers, identical in the 16 lanes of a row; cross-lane traffic is DPP inside a row
// (row_newbcast, quad_perm / row_mirror reductions) and one ds_bpermute where the source lane is data-dependent.
// Per root in LDS: the MDP as {uint16 local next state | bit 15 terminal[next]} + the rewards (f64), the tree, the path.
// Same trees, plans, statistics and generator records as every other variant.
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ double row16_max(double u) // every lane: the maximum over the 16 lanes of its DPP row
{
    u = max_step<0xB1, 0xf>(u);  // quad_perm:[1,0,3,2]
    u = max_step<0x4E, 0xf>(u);  // quad_perm:[2,3,0,1]
    u = max_step<0x141, 0xf>(u); // row_half_mirror
    u = max_step<0x140, 0xf>(u); // row_mirror
    return u;
}
// the maximum over lanes 0 .. |A| - 1 of a row (the lanes that score a level's children; the others hold -inf), in every one of them
template <int AT>
__device__ __forceinline__ double row_children_max(double u)
{
    u = max_step<0xB1, 0xf>(u);                 // quad_perm:[1,0,3,2]
    if (AT > 2) u = max_step<0x4E, 0xf>(u);     // quad_perm:[2,3,0,1]
    if (AT > 4) u = max_step<0x141, 0xf>(u);    // row_half_mirror: lanes 0..7 <-> 7..0
    return u;
}
constexpr int kRowRoots = 4; // roots per wavefront
// SHARED (later in round 6): the same kernel for ONE model shared by every root -- SURVEY 8(d)'s own batch, 4096 roots of the
// headline table.  uct_kernel<.., QD> keeps that model's compact tables in LDS (150 of 160 KB) and so has to leave the trees in
// global memory: a dependent L2 round trip per scored level and per backed-up node, a third of a small plan.  Here the workgroup
// stages ONE copy of the transitions (uint16 next | terminal bit: 2 B per (s, a), 100 KB for S = 10 000) and the sixteen trees
// of its four wavefronts take the place of the reward tables; a step's reward comes from the model's 16-byte records in L2 --
// requested when the state chain reaches the step, added to the return IN ORDER one level later (selection) or after the round
// of sixteen steps (rollout), so its latency is paid once per round, not per step.
template <int AT, bool SHARED = false>
__global__ __launch_bounds__(SHARED ? 1024 : 256) void uct_row_kernel(UctArgs p)
{
    static_assert(AT >= 2 && AT <= 8, "|A| with a compile-time specialisation");
    constexpr int A = AT, NTH = AT - 1;
    extern __shared__ __attribute__((aligned(16))) double lds_d[];
    // (a workgroup is blockDim.x / 64 wavefronts sharing one copy of the per-call tables; tools/wave_placement.hip: the dispatcher
    // spreads single-wave workgroups over the SIMDs just as well -- 1024 of them land one per SIMD -- so 1, 2 or 4 waves per
    // workgroup run at the same speed)
    // SHARED: a workgroup of sixteen wavefronts stages the model; p.waves of them stay to plan (four roots each)
    const int tid = threadIdx.x, lane = tid & 63, l16 = tid & 15, nthreads = blockDim.x;
    // SHARED: p.lanes = roots per wavefront, 4 or 2 (two: rows 2 and 3 of every wave idle -- twice the waves for the same roots,
    // two per SIMD, which fill each other's issue gaps; their lanes alias the wave's last live row and write nothing)
    const int rpw = SHARED ? p.lanes : kRowRoots;
    const int nrows = SHARED ? p.waves * rpw : nthreads >> 4;         // roots of this workgroup
    const bool row_used = !SHARED || ((tid >> 4) & 3) < rpw;
    const int row = SHARED ? min((tid >> 6) * rpw + min((tid >> 4) & 3, rpw - 1), nrows - 1) : tid >> 4;
    const int H = p.horizon, E = p.episodes, TE = p.table_n;
    double *gpow = lds_d;                   // [H + 1]  gamma ** h
    double *tp = gpow + (H + 1) + A;        // [A]      temperature * |A| * prior[a]
    double *rcp = tp + A;                   // [TE + 1]  1.0 / n
    double *tpdiv = rcp + (TE + 1);         // [A][TE+2] temperature * |A| * prior[a] / n
    const int ntab = (H + 1) + 2 * A + (TE + 1) + A * (TE + 2);
    const int ntab2 = (ntab + 1) & ~1;
    // (SHARED: no reward tables, one transition table for the workgroup)
    const int SA = (SHARED ? p.S : p.Sb) * A, SA2 = SHARED ? 0 : (SA + 1) & ~1, SA8 = (SA + 7) & ~7, PH = (H + 4) & ~3;
    double *rew = lds_d + ntab2 + row * SA2;                                                    // [rows][SA2] rewards
    UctNode *tnode = reinterpret_cast<UctNode *>(lds_d + ntab2 + nrows * SA2) + row * p.cap;    // [rows][cap] trees
    uint32_t *jump = reinterpret_cast<uint32_t *>(reinterpret_cast<UctNode *>(lds_d + ntab2 + nrows * SA2) + nrows * p.cap); // [H + 5][8]
    int32_t *path = reinterpret_cast<int32_t *>(jump + (H + 5) * 8) + row * PH;                 // [rows][PH] path node ids
    uint16_t *t16 = reinterpret_cast<uint16_t *>(reinterpret_cast<int32_t *>(jump + (H + 5) * 8) + nrows * PH) + (SHARED ? 0 : row * SA8); // [rows][SA8]
    const int r = blockIdx.x * nrows + row;
    const bool live = row_used && r < p.n_roots; // (a last wavefront's spare rows run along on the last root's data and write nothing)
    const int rr = live ? r : p.n_roots - 1;
    const int32_t s0g = p.root_state[rr];     // global state of the batch model
    const int32_t sbase = SHARED ? 0 : (s0g / p.Sb) * p.Sb; // first global state of this root's MDP
    for (int i = tid; i < (H + 5) * 8; i += nthreads) jump[i] = p.jump[i];
    for (int i = tid; i < ntab; i += nthreads) lds_d[i] = p.tab[i];
    if (SHARED) {
        // the model's compact transitions (pack_t16: next | terminal[next] << 15), 16 bytes a lane where the tail allows
        const int n8 = SA >> 3;
        const uint4 *src = reinterpret_cast<const uint4 *>(p.t16);
        uint4 *dst = reinterpret_cast<uint4 *>(t16);
#pragma unroll 4
        for (int i = tid; i < n8; i += nthreads) dst[i] = src[i];
        for (int i = (n8 << 3) + tid; i < SA; i += nthreads) t16[i] = p.t16[i];
    } else {
        const Rec *src = p.rec + (long)sbase * A;
#pragma unroll 4
        for (int i = l16; i < SA; i += 16) {
            const Rec rc = src[i];
            t16[i] = (uint16_t)((uint32_t)(rc.next - sbase) | ((rc.flags & 2u) ? 0x8000u : 0u));
            rew[i] = rc.reward;
        }
    }
    // SHARED: reward[s, a] from the 16-byte record in global memory (L2-resident: 16 S |A| bytes)
    auto reward_of = [&](unsigned idx) -> double { return SHARED ? p.rec[idx].reward : rew[idx]; };
    __syncthreads();
    if (SHARED && tid >= p.waves * 64) return;          // (the staging wavefronts)
    auto explore = [&](int a, int cnt1) { return cnt1 <= TE + 1 ? tpdiv[a * (TE + 2) + cnt1] : tp[a] / (double)cnt1; };
    auto inv = [&](int c) { return c <= TE ? rcp[c] : 1.0 / (double)c; };
    auto lds_sync = [] { // this wave's LDS writes before its later reads, for the compiler (the hardware keeps a wave's LDS order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    Pcg64 g;                                  // (the 16 lanes of a row hold the same generator)
    g.load(p.rng + (long)rr * 6);
    const int32_t s0 = s0g - sbase;
    const int32_t st0 = p.root_steps ? p.root_steps[rr] : 0;
    const bool root_term = (p.rec[(long)s0g * A].flags & 1u) != 0; // terminal flag of the root state itself ("source" rule)
    int n_nodes = 1, steps_taken = 0;
    if (l16 == 0 && row_used) { UctNode n; n.value = 0.0; n.count = 0; n.first_child = -1; tnode[0] = n; path[0] = 0; } // mcts.py:129-130 reset()
    lds_sync();
    const int la = l16 < A ? l16 : 0;
    const int row_lane0 = lane & 48;
    // the first round of a rollout's draws (lane l: the generator l + 1 steps ahead = A^(l+1) state + inc G_(l+1)): the limbs of
    // A^(l+1) and the product inc G_(l+1) are the same for every rollout of the plan -- registers, one 128-bit multiply per round
    uint32_t an0[4];
    uint64_t ig0_lo, ig0_hi;
    {
        const int j1 = l16 + 1 < H ? l16 + 1 : H;
        uint32_t gn0[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { an0[i] = jump[j1 * 8 + i]; gn0[i] = jump[j1 * 8 + 4 + i]; }
        Pcg64::mul128v(g.inc_lo, g.inc_hi, gn0, ig0_lo, ig0_hi);
    }
#ifdef MP_PROFILE
    long long t_sel = 0, t_exp = 0, t_draw = 0, t_walk = 0, t_cap = 0, t_bak = 0, n_lvl = 0, n_rounds = 0;
    const long long t_all0 = clock64();
#endif
    for (int ep = 0; ep < E; ++ep) { // mcts.py:179-184
        PROF_T(c0);
        int32_t s = s0, st = st0;
        int node = 0, depth = 0;
        bool terminal = false, cur_term = root_term;
        double total = 0.0;
        int fc = tnode[0].first_child;
        // SHARED: the reward of a scored level arrives from L2 while the next level is scored; it is added before that level's own
        // (same order of additions).  pend_w = gamma ** depth * [a reward is pending], pend_r = that reward.
        double pend_r = 0.0, pend_g = 0.0;
        bool pend = false;
        // ---- selection, mcts.py:143-149: a level's children one per lane of the row
        bool sel = live && depth < H && fc >= 0 && !terminal;
        while (any64(sel)) {
            const UctNode c = tnode[sel ? fc + la : 0];
            double sc = c.value + explore(la, c.count + 1);   // MCTSNode.selection_strategy, mcts.py:275-286
            if (l16 >= A) sc = -INFINITY;
            const double m = row_children_max<AT>(sc);
            const unsigned long long ball = ballot64(l16 < A && sc == m); // Node.random_argmax, abstract.py:296-311
            unsigned t = (unsigned)(ball >> row_lane0) & 0xffffu;
            const int nt = __popc(t);
            if (any64(sel && nt > 1)) {   // (no row of this wavefront has a tie: no draw, the first maximum is the only one)
                int pick = 0;
                if (sel && nt > 1) pick = (int)g.below((uint32_t)nt);
#pragma unroll
                for (int k = 0; k < A - 1; ++k)
                    if (pick > 0) { t &= t - 1; --pick; }
            }
            const int act = t ? __ffs((int)t) - 1 : 0;
            const unsigned idx = __umul24((unsigned)s, (unsigned)A) + (unsigned)act;
            // the chosen child's first_child, the transition, the reward and gamma ** depth: ONE LDS round trip
            const int nfc = tnode[sel ? fc + act : 0].first_child;
            const uint32_t e = t16[idx];
            const double rw = reward_of(idx), gp = gpow[depth];
            if (SHARED) {
                if (pend) total += pend_g * pend_r;       // the previous level's reward (requested a level ago)
                pend = sel; pend_r = rw; pend_g = gp;
            }
            if (sel) {
                if (!SHARED) total += gp * rw;
                const bool next_term = (e & 0x8000u) != 0;
                terminal = p.done_on_next ? next_term : cur_term;
                cur_term = next_term;
                s = (int32_t)(e & 0x7fffu);
                ++st; ++steps_taken;
                node = fc + act;
                ++depth;
                if (l16 == 0) path[depth] = node;
                fc = nfc;
            }
            sel = sel && depth < H && fc >= 0 && !terminal;
#ifdef MP_PROFILE
            ++n_lvl;
#endif
        }
        if (SHARED && pend) total += pend_g * pend_r;     // the last scored level's reward
        PROF_T(c1);
        // ---- expansion, mcts.py:151-154 / 237-246
        if (live && fc < 0 && depth < H && (!terminal || node == 0)) {
            if (l16 == 0) tnode[node].first_child = n_nodes;
            if (l16 < A) {
                UctNode n;
                n.value = 0.0; n.count = 0; n.first_child = -1;
                tnode[n_nodes + l16] = n;
            }
            n_nodes += A;
        }
        PROF_T(c2);
        // ---- rollout, mcts.py:156-157 / 160-177: rounds of 16 draws (one per lane of the row, by jump-ahead) and 16 steps of the walk
        const bool want = live && !terminal && depth < H;
        if (any64(want)) {
            int n_lim = H - depth;
            if (p.max_steps > 0 && p.max_steps - st < n_lim) n_lim = p.max_steps - st;
            if (n_lim < 1) n_lim = 1; // (the first step is unconditional, as in the reference's loop)
            bool alive = want, captured = false;
            int n = 0;
            for (int k16 = 0; any64(alive); k16 += 16) {
                PROF_T(d0);
                Pcg64 q = g;
                uint32_t act_l;
                {
                    if (k16 == 0) {
                        uint64_t p_lo, p_hi;
                        Pcg64::mul128v(g.s_lo, g.s_hi, an0, p_lo, p_hi);
                        const uint64_t lo = p_lo + ig0_lo;
                        q.s_hi = p_hi + ig0_hi + (lo < p_lo ? 1ULL : 0ULL);
                        q.s_lo = lo;
                    } else {
                        const int j1 = k16 + l16 + 1 < H ? k16 + l16 + 1 : H; // (draws beyond the horizon are never used)
                        uint32_t an[4], gn[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) { an[i] = jump[j1 * 8 + i]; gn[i] = jump[j1 * 8 + 4 + i]; }
                        q.jump(an, gn);
                    }
                    const uint64_t u = q.output();     // searchsorted(cdf, u, 'right') on the raw 64-bit output
                    int act = 0;
#pragma unroll
                    for (int a = 0; a < NTH; ++a) act += p.thr_arg[a] <= u ? 1 : 0;
                    act_l = (uint32_t)min(act, p.thr_valid);
                }
                PROF_T(d1);
                // SHARED: the rewards of the round's steps are requested as the state chain reaches them and summed afterwards, in
                // step order (a root's live steps are a prefix of the round: n_before .. n - 1)
                double rwv[16];
                const int n_before = n;
                // The walk in GROUPS OF FOUR steps, two passes each.  Pass 1 is the state chain alone -- index -> LDS read -> mask, four
                // times, SPECULATIVE: sw steps through the model whether or not the row's rollout is still running (a finished row reads
                // valid records nobody uses) -- with the rewards requested on the way.  Pass 2 is what the four steps mean for the rows
                // still rolling (terminal flags, step limit, the committed state and return).  A lone wave issues in order: with the
                // bookkeeping between two steps of the chain (the first form) every step paid for both.
                int32_t sw = s;
                uint32_t e4[4];
                double rw4[4];
#define MP_ROW_CHAIN(i_, j_)                                                                            \
    {                                                                                                   \
        const int a_i = dpp_mov<0x150 + (i_)>((int)act_l);      /* row_newbcast: lane i_ of the row */   \
        const unsigned idx = __umul24((unsigned)sw, (unsigned)A) + (unsigned)a_i;                       \
        e4[j_] = t16[idx];                                                                              \
        if (SHARED) rwv[i_] = reward_of(idx); else rw4[j_] = rew[idx];                                  \
        sw = (int32_t)(e4[j_] & 0x7fffu);                                                               \
    }
// pass 2, for the group as a whole: which of its four steps the row takes follows from four bits -- the terminal flags of the
// states reached -- and the step limit, so the per-step if / select chain (fifteen instructions a step) becomes bit arithmetic:
// stop bit j = "the rollout ends AFTER step j"; k = the steps taken = first stop bit + 1 (or 4).  The return's additions are the
// reference's, in order: a step not taken adds +0.0, which changes no bit of a sum that is never -0.
#define MP_ROW_BOOK4()                                                                                  \
    {                                                                                                   \
        const uint32_t nt = ((e4[0] >> 15) & 1u) | ((e4[1] >> 14) & 2u) | ((e4[2] >> 13) & 4u) | ((e4[3] >> 12) & 8u);  \
        const uint32_t th = p.done_on_next ? nt : (((nt << 1) | (cur_term ? 1u : 0u)) & 15u);           \
        const int left = n_lim - n;                              /* steps still allowed: >= 1 while alive */ \
        const uint32_t lim = left <= 4 ? 1u << ((left - 1) & 3) : 0u;                                   \
        const uint32_t stop = th | lim;                                                                 \
        const int first = stop ? __ffs((int)stop) - 1 : 4;                                              \
        const int k = alive ? min(first + 1, 4) : 0;                                                    \
        if (!SHARED) {                                                                                  \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                             \
                const double add = gpow[min(depth + n + j, H)] * rw4[j];                                \
                total += j < k ? add : 0.0;                                                             \
            }                                                                                           \
        }                                                                                               \
        const uint32_t ek = k <= 1 ? e4[0] : (k == 2 ? e4[1] : (k == 3 ? e4[2] : e4[3]));               \
        s = k > 0 ? (int32_t)(ek & 0x7fffu) : s;                                                        \
        cur_term = k > 0 ? (ek & 0x8000u) != 0 : cur_term;                                              \
        n += k;                                                                                         \
        alive = alive && first >= 4;                                                                    \
    }
#define MP_ROW_WALK4(g_)                                                                                \
    MP_ROW_CHAIN(4 * (g_), 0) MP_ROW_CHAIN(4 * (g_) + 1, 1) MP_ROW_CHAIN(4 * (g_) + 2, 2) MP_ROW_CHAIN(4 * (g_) + 3, 3)     \
    MP_ROW_BOOK4()
                int groups = 1;                                   // groups of four this round walked (wave-uniform)
                MP_ROW_WALK4(0)
                if (any64(alive)) {
                    groups = 2;
                    MP_ROW_WALK4(1)
                    if (any64(alive)) {
                        groups = 3;
                        MP_ROW_WALK4(2)
                        if (any64(alive)) { groups = 4; MP_ROW_WALK4(3) }
                    }
                }
#undef MP_ROW_WALK4
#undef MP_ROW_BOOK4
#undef MP_ROW_CHAIN
                if (SHARED) {
                    // the round's return, in step order, over the groups that were walked; a step the row did not take adds +0.0
                    const int taken = n - n_before;
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        if (gq < groups) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int i = 4 * gq + j;
                                const double add = gpow[min(depth + n_before + i, H)] * rwv[i];
                                total += i < taken ? add : 0.0;
                            }
                        }
                    }
                }
                PROF_T(d2);
                // a row whose rollout ended in this round: its generator after the n draws it consumed = the state the lane of
                // its last draw jumped to
                const int src = (row_lane0 + ((n - 1) & 15)) << 2;
                const uint32_t x0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)q.s_lo);
                const uint32_t x1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(q.s_lo >> 32));
                const uint32_t x2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)q.s_hi);
                const uint32_t x3 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(q.s_hi >> 32));
                if (want && !alive && !captured) {
                    g.s_lo = ((uint64_t)x1 << 32) | x0;
                    g.s_hi = ((uint64_t)x3 << 32) | x2;
                    captured = true;
                }
#ifdef MP_PROFILE
                { const long long d3 = clock64(); t_draw += d1 - d0; t_walk += d2 - d1; t_cap += d3 - d2; ++n_rounds; }
#endif
            }
            if (want) { st += n; steps_taken += n; }
        }
        PROF_T(c3);
        // ---- backup, mcts.py:248-265: the same return for every node on the path, one node per lane of the row
        lds_sync();
        for (int d0 = 0; any64(live && d0 <= depth); d0 += 16) {
            const int d = d0 + l16;
            if (live && d <= depth) {
                const int nd = path[d];
                UctNode c = tnode[nd];
                c.count += 1;
                c.value += inv(c.count) * (total - c.value);
                tnode[nd].value = c.value;       // (first_child is left alone: the node may just have been expanded)
                tnode[nd].count = c.count;
            }
        }
        lds_sync();
#ifdef MP_PROFILE
        { const long long c4 = clock64(); t_sel += c1 - c0; t_exp += c2 - c1; t_bak += c4 - c3; }
#endif
    }
#ifdef MP_PROFILE
    if (blockIdx.x == 0 && lane == 0)
        printf("uct_row prof wave0: total=%lld select=%lld (levels %lld) expand=%lld draw=%lld walk=%lld capture=%lld (rounds %lld) backup=%lld\n",
               (long long)(clock64() - t_all0), t_sel, n_lvl, t_exp, t_draw, t_walk, t_cap, n_rounds, t_bak);
#endif
    if (!live) return;
    // the tree, to global memory in the group-interleaved layout (export, re-rooting by step_by_subtree)
    const TreeRef<2, AT> tree = tree_of<2, AT>(p.tree, r, p.cap, A);
    for (int i = l16; i < n_nodes; i += 16) tree[i] = tnode[i];
    if (l16 == 0) {
        g.store(p.rng + (long)r * 6);
        // ---- AbstractPlanner.get_plan (abstract.py:143-156) with MCTSNode.selection_rule (mcts.py:212-218): most visited
        // child, ties -> first maximal value among them
        int len = 0;
        int fc = tnode[0].first_child;
        while (fc >= 0) {
            int mc = tnode[fc].count;
            for (int a = 1; a < A; ++a) mc = max(mc, tnode[fc + a].count);
            int best = -1;
            double bv = 0.0;
            for (int a = 0; a < A; ++a) {
                const UctNode c = tnode[fc + a];
                if (c.count == mc && (best < 0 || c.value > bv)) { best = a; bv = c.value; }
            }
            if (p.plans && len < p.max_plan_len) p.plans[(long)r * p.max_plan_len + len] = best;
            ++len;
            fc = tnode[fc + best].first_child;
        }
        if (p.plans)
            for (int i = len; i < p.max_plan_len; ++i) p.plans[(long)r * p.max_plan_len + i] = -1;
        if (p.plan_len) p.plan_len[r] = len;
        if (p.n_nodes_out) p.n_nodes_out[r] = n_nodes;
        if (p.root_value) p.root_value[r] = tnode[0].value;
        if (p.env_steps) p.env_steps[r] = (int64_t)steps_taken;
        const int rfc = tnode[0].first_child;
        for (int a = 0; a < A; ++a) {
            if (p.root_child_count) p.root_child_count[(long)r * A + a] = rfc >= 0 ? max(tnode[rfc + a].count, 0) : 0;
            if (p.root_child_value) p.root_child_value[(long)r * A + a] = rfc >= 0 ? tnode[rfc + a].value : 0.0;
        }
    }
}

// one thread: the visit count at the end of an action path (mp_uct_path_count)
// `virgin` (UctTreeMode, uct_virgin.hpp): the children of a count-1 node, or the children whose bit in the parent's word is clear,
// were never stored -- a path that enters one ends at a node of count 0 without children
template <int IL>
__global__ void uct_path_count_kernel(UctNode *trees, int root, int cap, int A, const int32_t *actions, int n, int64_t *out, int virgin)
{
    const TreeRef<IL, 0> tree = tree_of<IL, 0>(trees, root, cap, A);
    int node = 0;
    bool unstored = false; // `node` was never stored
    for (int i = 0; i < n; ++i) {
        const int w = unstored ? -1 : tree[node].first_child;
        const int fc = virgin == kUctTreeMasked ? uct_word_child(w) : w;
        const int a = actions[i];
        if (fc < 0 || a < 0 || a >= A) { out[0] = -1; return; }
        unstored = virgin == kUctTreeMasked ? !uct_word_stored(w, a) : (virgin == kUctTreeCount1 && tree[node].count == 1);
        node = fc + a;
    }
    const int c = unstored ? 0 : tree[node].count;
    out[0] = c < 0 ? -1 : c; // (count < 0: the phantom slot of an action a listed policy does not list)
}

// AbstractPlanner.step_by_subtree (abstract.py:195-206), one root per lane: the subtree of the root's child
// `action` is re-numbered breadth-first into the other tree buffer (children stay contiguous).  While a node
// waits in the BFS queue its first_child field holds its OLD id.  A never-expanded root gives size 0 (fresh tree).
// `source` (mp_uct_step_tree_select): new root r continues OLD root source[r] of the n_src old ones -- in any order, one source
// for several new roots, a source outside the old batch = a fresh tree; then n_new is another array than n_old (a new root's
// size must not overwrite an old root's before every lane has read its own).  source == nullptr: root r continues root r.
template <int IL>
__global__ __launch_bounds__(64) void uct_reroot_kernel(int n_roots, int n_src, int A, int cap_old, int cap_new,
                                                        const UctNode *__restrict__ old_trees, UctNode *__restrict__ new_trees,
                                                        const int32_t *n_old, const int32_t *__restrict__ source,
                                                        const int32_t *__restrict__ actions,
                                                        int32_t *n_new, // (n_old and n_new are the same array when source == nullptr)
                                                        int virgin) // which nodes of the old trees were never stored (UctTreeMode, uct_virgin.hpp); the new ones are whole
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_roots) return;
    const int q = source ? source[r] : r;
    if (q < 0 || q >= n_src) {
        n_new[r] = 0;
        return;
    }
    const TreeRef<IL, 0> o = tree_of<IL, 0>(const_cast<UctNode *>(old_trees), q, cap_old, A); // (generic ids: operator[])
    const TreeRef<IL, 0> n = tree_of<IL, 0>(new_trees, r, cap_new, A);
    const int a = actions[r];
    // `if action in self.root.children` (abstract.py:201): an unlisted action has a phantom slot, not a child
    // (a masked tree's root holds the full mask: its children are all stored)
    const int rfc = n_old[q] < 1 ? -1 : (virgin == kUctTreeMasked ? uct_word_child(o[0].first_child) : o[0].first_child);
    if (rfc < 0 || a < 0 || a >= A || o[rfc + a].count < 0) {
        n_new[r] = 0;
        return;
    }
    int head = 0, tail = 1;
    UctNode first;
    first.first_child = rfc + a;
    n[0] = first;
    while (head < tail) {
        const int oid = n[head].first_child; // (-2: a node of the old tree that was never stored -- the constant node)
        UctNode src;
        src.value = 0.0; src.count = 0; src.first_child = -1;
        if (oid >= 0) src = o[oid];
        UctNode out;
        out.value = src.value; out.count = src.count; out.first_child = -1;
        if (src.first_child >= 0) {
            out.first_child = tail;
            const int sfc = virgin == kUctTreeMasked ? uct_word_child(src.first_child) : src.first_child;
            for (int c = 0; c < A; ++c) {
                const bool unstored = virgin == kUctTreeMasked ? !uct_word_stored(src.first_child, c)
                                                               : (virgin == kUctTreeCount1 && src.count == 1);
                UctNode q;
                q.value = 0.0; q.count = 0; q.first_child = unstored ? -2 : sfc + c;
                n[tail + c] = q;
            }
            tail += A;
        }
        n[head] = out;
        ++head;
    }
    n_new[r] = tail;
}

// ---- per-state policies fused ON THE DEVICE (round 6).  mp_policy_load's host loops (download the model's records, S * |A|
// thresholds and fused records in C++, six hipMalloc'ed arrays uploaded) cost 90 ms per call on the batch model of 4096
// highway episodes (491 520 global states) -- per step of the per-episode evaluation loop, whose tables change at every step.
// The same arithmetic as kernels: one thread per state for the prior row, the sampling thresholds ceil(cdf * 2^53) (numpy's
// cumsum order, IEEE division) and the listed-action mask; one thread per (s, a) for the fused record.  `rows` < S: the
// distributions are given for ONE MDP of a batch model (local states) and apply to every MDP -- the planner's own policies on a
// batch of environments that restrict their actions identically.
struct PolBuild {
    int S, A, stride, frq, rows, shift, can_pack;
    const double *prior, *rollout;   // [rows][A]
    const uint8_t *listed, *slot;    // [rows][A] or nullptr
    const Rec *rec;                  // [S * A]
    double *hp;                      // [S][stride]
    uint64_t *ht;                    // [S][stride]
    uint32_t *lmask;                 // [S]
    uint32_t *hf, *hfr, *hp16;       // [S * A][frq * 4], the same by rollout slot (or nullptr), [S * A][4] (or nullptr)
    int32_t *err;                    // {code, state}: 1 negative / NaN probability, 2 rollout row sums to 0, 3 no listed action,
                                     // 4 rollout slots not a permutation, 5 transition out of range
};
__device__ __forceinline__ void pol_err(const PolBuild &b, int code, int s)
{
    if (atomicCAS(b.err, 0, code) == 0) b.err[1] = s;
}
__global__ void policy_rows_kernel(PolBuild b)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= b.S) return;
    const int A = b.A, r = s % b.rows;
    double cdf[8];
    double acc = 0.0;
    unsigned seen = 0;
    for (int a = 0; a < A; ++a) {
        const int c = b.slot ? (int)b.slot[(size_t)r * A + a] : a;
        if (c >= A || ((seen >> c) & 1u)) { pol_err(b, 4, s); return; }
        seen |= 1u << c;
        const double q = b.rollout[(size_t)r * A + c], pr = b.prior[(size_t)r * A + a];
        if (!(q >= 0.0) || !(pr >= 0.0)) pol_err(b, 1, s);
        b.hp[(size_t)s * b.stride + a] = pr;
        acc += q; cdf[a] = acc;                                                    // numpy cumsum, in the rollout policy's order
    }
    if (!(acc > 0.0)) pol_err(b, 2, s);
    for (int a = 0; a < A; ++a) {
        const double scaled = ceil((cdf[a] / acc) * 9007199254740992.0);           // cdf /= cdf[-1]; ceil(ldexp(., 53))
        b.ht[(size_t)s * b.stride + a] = scaled >= 18446744073709551615.0 ? ~0ULL : (uint64_t)scaled;
    }
    for (int a = A; a < b.stride; ++a) { b.hp[(size_t)s * b.stride + a] = 0.0; b.ht[(size_t)s * b.stride + a] = ~0ULL; }
    uint32_t m = (1u << A) - 1u;
    if (b.listed) {
        m = 0;
        for (int a = 0; a < A; ++a) m |= (b.listed[(size_t)r * A + a] ? 1u : 0u) << a;
        if (!m) pol_err(b, 3, s);
    }
    b.lmask[s] = m;
}
__global__ void policy_frec_kernel(PolBuild b)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)b.S * b.A) return;
    const int A = b.A;
    uint32_t *f = b.hf + (size_t)i * b.frq * 4;
    const uint4 rc = reinterpret_cast<const uint4 *>(b.rec)[i];
    const int nx = (int)rc.x;
    if (nx < 0 || nx >= b.S) { pol_err(b, 5, (int)(i / A)); return; }
    f[0] = rc.x; f[2] = rc.z; f[3] = rc.w;
    f[1] = (rc.y & 0xffu) | (b.lmask[nx] << 8) | (b.lmask[i / A] << 16);
    for (int k = 4; k < b.frq * 4; ++k) f[k] = 0xffffffffu;
    uint32_t th[4] = {1023u, 1023u, 1023u, 1023u};
    for (int a = 0; a + 1 < A; ++a) {
        const uint64_t t53 = b.ht[(size_t)nx * b.stride + a];
        const uint64_t hi = t53 >> b.shift;                                        // top bits of the 53, saturated
        f[4 + a] = hi > 0xffffffffULL ? 0xffffffffu : (uint32_t)hi;
        if (b.can_pack && a < 4) th[a] = (t53 >> 43) > 1023ULL ? 1023u : (uint32_t)(t53 >> 43);
    }
    if (b.can_pack) {
        uint32_t *g = b.hp16 + (size_t)i * 4;
        g[0] = (uint32_t)nx | (th[0] << 20);
        g[1] = (rc.y & 3u) | (th[1] << 2) | (th[2] << 12) | (th[3] << 22);
        g[2] = rc.z; g[3] = rc.w;
    }
}
__global__ void policy_froll_kernel(PolBuild b) // entry (s, k) = the record of (s, column of slot k)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)b.S * b.A) return;
    const int s = (int)(i / b.A), k = (int)(i % b.A), r = s % b.rows;
    const int c = b.slot[(size_t)r * b.A + k];
    if (c >= b.A) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(b.hf) + ((size_t)s * b.A + c) * b.frq;
    uint4 *dst = reinterpret_cast<uint4 *>(b.hfr) + (size_t)i * b.frq;
    for (int q = 0; q < b.frq; ++q) dst[q] = src[q];
}

} // namespace mp

using namespace mp;

// Apply the re-rooting armed by mp_uct_step_tree / mp_uct_step_tree_select (reroot_apply) to the trees of the last mp_uct_plan,
// into the other tree workspace with node stride cap_new.
static int uct_reroot_now(mp_ctx *ctx, long cap_new)
{
    const int n_roots = ctx->tree.n_roots;
    const int old_slot = ctx->tree.buf ? WS_TREE2 : WS_TREE0, new_slot = ctx->tree.buf ? WS_TREE0 : WS_TREE2;
    UctNode *nw = nullptr;
    MP_TRY(ws_get(ctx, new_slot, (size_t)((n_roots + 63) & ~63) * tree_stride_alloc(ctx->tree.il, cap_new, ctx->tree.A), &nw));
    const int virgin = ctx->tree.virgin;
    ctx->tree.virgin = kUctTreeWhole; // (the re-rooted trees are whole, their words plain)
    return reroot_apply(ctx, cap_new, [&](const Reroot &r) {
        hipLaunchKernelGGL(ctx->tree.il == 2 ? uct_reroot_kernel<2> : uct_reroot_kernel<0>, dim3((unsigned)((r.n_roots + 63) / 64)), dim3(64), 0,
                           ctx->stream, r.n_roots, r.n_src, r.A, r.cap_old, r.cap_new, (const UctNode *)ctx->ws[old_slot].p, nw, r.sizes, r.src,
                           r.acts, r.sizes_new, virgin);
    });
}

// ---- which kernel form a plan takes, and its geometry: a pure host function of the call's shape, the model's and the
// policy's facts, the kept tree and the MP_UCT_* knobs.  No HIP call, no ctx: mp_uct_choose_form runs it without a device.
// DESIGN.md §4.1 tabulates the forms, their defaults and the knobs that force them.
enum UctForm { UF_GLOBAL, UF_GLOBAL_SPILL, UF_LDSR, UF_QUAD, UF_LONE, UF_LONE_MW, UF_LONE_EACH, UF_ROW_EACH, UF_ROW_SHARED,
               UF_CARTPOLE, UF_POLICY, UF_COUNT };
static_assert(UF_COUNT == kUctForms, "uct_form_name (form_names.hpp) names the forms in this order");

constexpr int kUnset = INT_MIN;
// the knobs that pick a form or its geometry (kUnset: not set), read once per call -- tests change them between calls
struct UctKnobs {
    int model;        // MP_UCT_MODEL: 1 "ldsr" (the LDS-resident form), 0 any other value (the gather form)
    int quad, lone, each, row, rows;   // MP_UCT_QUAD / LONE / EACH / ROW / ROWS: their atoi
    int lone_waves;   // MP_UCT_LONE_WAVES: 1 / 2 / 4 / 8, any other value 0 (off)
    int row_waves, row_roots, lanes, cart_rep, cart_waves;   // MP_UCT_ROW_WAVES / ROW_ROOTS / LANES / CART_REP / CART_WAVES
    int path;         // MP_UCT_PATH: 1 "spill" (the register / global path stack, a test hook), 0 any other value
    long ldsr_waves;  // MP_UCT_LDSR_WAVES (LONG_MIN: not set)
    int tree_stores;  // MP_UCT_TREE_STORES: 0 "lane" (the per-lane tree stores of uct_kernel, for A/B runs), 1 "group" (the wave's
                      // expansions and the leaf's single store, every zero group stored and loaded), 2 "virgin" (virgin groups
                      // neither loaded nor, in fresh trees, stored before their first entry: the count-1 rule of uct_virgin.hpp),
                      // 3 any other value or unset (fresh trees store and load only the children an episode picked: the visited
                      // mask of uct_virgin.hpp; a form or a tree that cannot keep it runs as 2)
    int balance;      // MP_UCT_BALANCE: 0 runs the LDS-resident form without its wave balance (every rollout at priority 0, for A/B
                      // runs and tests), any other value or unset with it
    int action_table; // MP_UCT_ACTION_TABLE: 0 runs the LDS-resident form with the exact compares in every rollout step (for A/B
                      // runs and tests), any other value or unset with the action table where it has room
};
static int uct_knob(const char *name)
{
    const char *e = getenv(name);
    return e ? atoi(e) : kUnset;
}
static UctKnobs uct_knobs_read()
{
    UctKnobs k;
    const char *model = getenv("MP_UCT_MODEL"), *path = getenv("MP_UCT_PATH"), *ldsr_waves = getenv("MP_UCT_LDSR_WAVES");
    k.model = model ? !strcmp(model, "ldsr") : kUnset;
    k.path = path ? path[0] == 's' : kUnset;
    k.ldsr_waves = ldsr_waves ? atol(ldsr_waves) : LONG_MIN;
    k.quad = uct_knob("MP_UCT_QUAD"); k.lone = uct_knob("MP_UCT_LONE"); k.each = uct_knob("MP_UCT_EACH");
    k.row = uct_knob("MP_UCT_ROW"); k.rows = uct_knob("MP_UCT_ROWS");
    k.lone_waves = uct_knob("MP_UCT_LONE_WAVES");
    if (k.lone_waves != kUnset && k.lone_waves != 1 && k.lone_waves != 2 && k.lone_waves != 4 && k.lone_waves != 8) k.lone_waves = 0;
    k.row_waves = uct_knob("MP_UCT_ROW_WAVES"); k.row_roots = uct_knob("MP_UCT_ROW_ROOTS"); k.lanes = uct_knob("MP_UCT_LANES");
    k.cart_rep = uct_knob("MP_UCT_CART_REP"); k.cart_waves = uct_knob("MP_UCT_CART_WAVES");
    const char *tree_stores = getenv("MP_UCT_TREE_STORES");
    k.tree_stores = !tree_stores ? 3 : (!strcmp(tree_stores, "lane") ? 0 : (!strcmp(tree_stores, "group") ? 1 : (!strcmp(tree_stores, "virgin") ? 2 : 3)));
    k.balance = uct_knob("MP_UCT_BALANCE") != 0;
    k.action_table = uct_knob("MP_UCT_ACTION_TABLE") != 0;
    return k;
}

// what the chooser needs to know of a call
struct UctCall {
    int n_roots, episodes, horizon, A, S, NB, Sb;   // (NB, Sb: the model's MDPs and states per MDP)
    bool t16, r8;   // the model has compact transitions / a compact reward index (then n_rdict distinct rewards)
    int n_rdict;
    bool cart, pol, listed;
    int kept_il;    // the layout of the kept tree this plan continues; -1: fresh trees
    int cus;        // compute units (<= 0: taken as 256)
};
// the choice: the form, the tree layout, the kernel arguments lanes / waves / rep_shift, the launch's roots and threads per
// workgroup and its dynamic LDS bytes
struct UctChoice {
    UctForm form;
    int tree_il, lanes, waves, rep_shift, roots_per_wg, threads;
    size_t lds;
};

static int uct_choose(const UctCall &c, const UctKnobs &k, UctChoice *out)
{
    const int A = c.A, H = c.horizon, E = c.episodes;
    const long n = c.n_roots, cus = c.cus > 0 ? c.cus : 256, cap = 1 + (long)E * A;
    const bool at_known = A >= 2 && A <= 8, fresh = c.kept_il < 0, forced = k.model != kUnset;
    // LDS bytes.  The per-call tables (their quotient tables hold 16 KB at most), arrays 16-byte aligned, transitions as uint16,
    // the generator's jump table (n = 0 .. H and the lanes' 1 .. 4), a path stack of [H + 1][64] per wavefront.
    const int te_max = (int)(16384 / (sizeof(double) * (size_t)(A + 1))), TE = E < te_max ? E : te_max;
    const size_t ntab = (size_t)(H + 1) + 2 * (size_t)A + (TE + 1) + (size_t)A * (TE + 2), tabs = ntab * sizeof(double);
    auto dbl16 = [](size_t m) { return ((m + 1) & ~(size_t)1) * sizeof(double); };
    auto t16_bytes = [](size_t m) { return ((m + 7) & ~(size_t)7) * 2; };
    const size_t sa = (size_t)c.S * A, sa_each = (size_t)(c.NB > 1 && c.Sb > 0 ? c.Sb : c.S) * A;
    const size_t jump = (size_t)(H + 5) * 32, path_stack = (size_t)(H + 1) * 64 * sizeof(int32_t);
    const size_t tree_lds = (size_t)cap * (sizeof(UctNode) + sizeof(double)) + (size_t)(H + 1) * sizeof(int32_t) + 16;
    const size_t lds_ldsr = dbl16(ntab) + dbl16(c.n_rdict) + t16_bytes(sa) + ((sa + 15) & ~(size_t)15);
    const size_t lds_quad = lds_ldsr + jump, lds_lone = lds_quad + tree_lds;
    const size_t lds_each = dbl16(ntab) + dbl16(sa_each) + t16_bytes(sa_each) + jump + tree_lds;
    auto lds_lone_mw = [&](int w) {     // tables + the transitions + w x (jump table + tree + exploration terms)
        return dbl16(ntab) + t16_bytes(sa) + (size_t)w * ((((size_t)(H + 5) * 8 + (size_t)cap * 6 + 3) & ~(size_t)3) * 4) + 16;
    };
    const size_t row_tree = (size_t)cap * sizeof(UctNode) + (size_t)((H + 4) & ~3) * sizeof(int32_t);
    auto lds_row_each = [&](int rows) { return dbl16(ntab) + jump + rows * (row_tree + dbl16(sa_each) + t16_bytes(sa_each)); };
    auto lds_row_shared = [&](int rows) { return dbl16(ntab) + jump + rows * row_tree + t16_bytes(sa); };

    // Which forms the call can take.  The LDS forms plan state-independent policies on table models with |A| in 2..8, and all
    // but the LDS-resident one and its four-lanes-per-root form start from fresh trees.
    const bool table = !c.cart && !c.pol && at_known;
    const bool resident = table && c.t16 && c.r8;                                // the whole model in 3 B per (s, a)
    const bool shared = table && c.t16 && c.NB <= 1 && fresh;                    // one model's transitions
    const bool batch = table && c.NB > 1 && c.Sb > 0 && c.Sb < 32768 && fresh;   // one MDP per root
    // LDS-RESIDENT model (transitions + reward indices + reward table in LDS, nothing of an env step in global memory).
    // Measured (headline table, 33 x 30; profiles/r04_uct_ldsr.md): kernel ms global / LDS-resident at 8 192 roots 0.342 / 0.357,
    // 32 768 0.376 / 0.383, 65 536 0.412 / 0.369, 131 072 0.564 / 0.473, 262 144 1.049 / 0.781, 524 288 2.050 / 1.545 -- staging
    // 150 KB per workgroup costs ~25 us and a lone wave per SIMD hides the gather anyway, so it is the default from one wave per
    // SIMD (four per CU) upwards.
    bool ldsr = resident && k.model != 0 && (forced || (n + 63) / 64 >= 4 * cus);
    if (ldsr && lds_ldsr > kLdsBytes) {
        if (forced) return fail(MP_ERR_ARG, "mp_uct_plan: model does not fit LDS (%zu B)", lds_ldsr);
        ldsr = false;
    }
    // FOUR LANES PER ROOT: at most one wave per SIMD's worth of roots (16 per wave: 16 384 roots on 256 CUs).  Measured
    // (profiles/r05_uct_small_batch.md): 64 .. 16 384 roots 1.2-1.25x faster than the one-lane-per-root gather kernel, a single
    // root level with it (0.186 against 0.183 ms: its chain is selection + backup in global memory).
    const bool quad = resident && H >= 1 && H <= 255 && lds_quad <= kLdsBytes &&
                      (k.quad != kUnset ? k.quad != 0 : !forced && n >= 16 && (n + 15) / 16 <= 4 * cus);
    // ONE ROOT PER WORKGROUP: batches of at most one root per CU -- a single agent's act() above all: model, tables AND tree in
    // LDS, the whole wavefront working for the root.  One workgroup per CU for a model that fills its LDS (the headline table:
    // 256 roots 0.088 ms); for smaller models as many as fit a CU's LDS together, up to two planning wavefronts per SIMD
    // (tools/uct_small_batch.py with UCT_SB_SHAPE, round 6: S = 1 000: 1 024 roots 0.068 ms against the row kernel's 0.090;
    // S = 250: 2 048 roots 0.083 / 0.094; S = 3 000: 512 roots 0.088 / 0.128 -- and slower than the rows as soon as the
    // workgroups need a second round).
    bool lone = resident && fresh && H >= 1 && H <= 63 && lds_lone <= kLdsBytes &&
                (k.lone != kUnset ? k.lone != 0 : !forced && k.quad == kUnset && n <= cus * std::min(std::max((long)(kLdsBytes / lds_lone), 1L), 8L));
    // ... and SEVERAL planning wavefronts per workgroup around one copy of the transitions, the rewards from the records in L2:
    // for a model that fills the LDS, batches of up to 8 roots per CU (two wavefronts per SIMD) -- and, with ONE planning
    // wavefront, small batches of a model the plain form cannot take (more than 256 distinct rewards, or transitions + reward
    // indices beyond the LDS; the transitions alone may still fit).
    int lone_w = 0;
    if (shared && H >= 1 && H <= 63 && (!lone || k.lone_waves > 0) && k.lone != 0) {
        if (k.lone_waves != kUnset) lone_w = k.lone_waves;
        else if (!forced && k.quad == kUnset && k.rows == kUnset && k.path == kUnset && n <= 8 * cus)
            lone_w = n <= cus ? 1 : (n <= 2 * cus ? 2 : (n <= 4 * cus ? 4 : 8));
        if (lone_w && lds_lone_mw(lone_w) <= kLdsBytes) lone = true;
        else lone_w = 0;
    }
    // ONE MDP PER ROOT: a batch model, every root's own MDP staged into its workgroup's LDS from the 16-byte records (10 B per
    // (s, a)), whatever the batch size ...
    const bool each = batch && H >= 1 && H <= 63 && lds_each <= kLdsBytes && !forced && k.each != 0;
    // ... and FOUR such roots per wavefront, a DPP row each, with four waves per workgroup (one per SIMD) while their MDPs + trees
    // fit the LDS, else two / one.  Measured (tools/each_ab.sh, S = 120, 33 x 30): a wavefront per root against four roots per
    // wavefront -- 256 roots 0.062 ms (lone), 512: 0.065 / 0.091, 1024: 0.067 / 0.090, 2048: 0.077 / 0.090, 4096: 0.143 / 0.098.
    // Up to two wavefronts per SIMD (and while their workgroups' LDS fits the CU together) a root is served best by a whole
    // wavefront; beyond, the rows win (the SIMD is 16 lanes wide: four lone waves run at a quarter each).
    int row_waves = k.row_waves == 1 || k.row_waves == 2 || k.row_waves == 4 ? k.row_waves : 4;
    while (row_waves > 1 && lds_row_each(kRowRoots * row_waves) > kLdsBytes) row_waves >>= 1;
    const bool rowk = batch && H >= 1 && H <= 255 && lds_row_each(kRowRoots * row_waves) <= kLdsBytes && !forced && k.each != 0 &&
                      k.row != 0 && (k.row != kUnset || !each || n > cus * std::min(std::max((long)(kLdsBytes / lds_each), 1L), 8L));
    // ... and the SHARED-model row form: batches between one root per CU and sixteen (one round of four-wave workgroups) of a model
    // whose transitions + the workgroup's trees fit the LDS.  Two roots per wavefront (rows 2 and 3 idle) while that still fits
    // one wave per SIMD: a wave's rounds then run to the slower of 2 roots instead of 4 (2048 roots 0.197 -> 0.187 ms, 1024 roots
    // 0.195 -> 0.184); two such waves per SIMD for 4096 roots measure the same as one wave of four (0.201 against 0.197).  As few
    // waves per workgroup as still put the batch on the chip in one round (fewer roots behind one staged copy).
    const int rpw = n <= 2L * 4 * cus ? 2 : kRowRoots;
    int rowsh_waves = 4;
    while (rowsh_waves > 1 && (n + rpw * (rowsh_waves / 2) - 1) / (rpw * (rowsh_waves / 2)) <= cus) rowsh_waves >>= 1;
    if (k.row_waves == 1 || k.row_waves == 2 || k.row_waves == 4 || k.row_waves == 8) rowsh_waves = k.row_waves;
    const int rowsh_rpw = k.row_roots == 2 || k.row_roots == 4 ? k.row_roots : rpw;
    while (rowsh_waves > 1 && lds_row_shared(rowsh_rpw * rowsh_waves) > kLdsBytes) rowsh_waves >>= 1;
    const bool rowsh = shared && H >= 1 && H <= 255 && lds_row_shared(rowsh_rpw * rowsh_waves) <= kLdsBytes && !forced && !rowk && !each &&
                       (k.rows != kUnset ? k.rows != 0 : !lone && k.quad == kUnset && k.path == kUnset && n >= 16 && n <= 4L * kRowRoots * cus);

    UctChoice o;
    o.form = c.cart ? UF_CARTPOLE : c.pol ? UF_POLICY : rowsh ? UF_ROW_SHARED : rowk ? UF_ROW_EACH : each ? UF_LONE_EACH
           : lone ? (lone_w ? UF_LONE_MW : UF_LONE) : quad ? UF_QUAD : ldsr ? UF_LDSR : UF_GLOBAL;
    o.tree_il = fresh ? (c.cart || !at_known ? 0 : 2) : c.kept_il;
    // a kept tree in another layout than the LDS-resident forms': the default kernel with its LDS budget (MP_UCT_PATH aside)
    const bool fallback = (o.form == UF_LDSR || o.form == UF_QUAD) && o.tree_il != 2;
    if (fallback) o.form = UF_GLOBAL;
    // Roots per wavefront of the other forms.  A root's episodes are one long dependency chain, so a batch takes as long as its
    // slowest wavefront; measured on MI355X (4096 roots, highway table) dense waves are fastest: 64 lanes 0.41 ms, 16 lanes
    // 0.44 ms, 4 lanes 0.70 ms.
    o.lanes = k.lanes == 1 || k.lanes == 2 || k.lanes == 4 || k.lanes == 8 || k.lanes == 16 || k.lanes == 32 ? k.lanes : 64;
    o.waves = 1; o.rep_shift = 0;
    o.roots_per_wg = 1; o.threads = 1024;
    switch (o.form) {
    case UF_LDSR:
    case UF_QUAD: {
        // one workgroup per CU shares the tables: as many waves per workgroup as it takes to put the batch on the chip's CUs (a
        // power of two <= 16, so that chunk boundaries -- multiples of 1024 roots -- are workgroup boundaries)
        o.lanes = o.form == UF_QUAD ? 16 : 64;
        const long w = k.ldsr_waves != LONG_MIN ? k.ldsr_waves : ((n + o.lanes - 1) / o.lanes + cus - 1) / cus;
        while (o.waves < w && o.waves < 16) o.waves <<= 1;
        o.lds = o.form == UF_QUAD ? lds_quad : lds_ldsr;
        break;
    }
    case UF_LONE: o.lds = lds_lone; break;
    case UF_LONE_MW: o.waves = o.roots_per_wg = lone_w; o.lds = lds_lone_mw(lone_w); break;
    case UF_LONE_EACH: o.threads = sa_each <= 4096 ? 64 : 256; o.lds = lds_each; break;   // (one wave while it stages its MDP in a few trips)
    case UF_ROW_EACH: o.roots_per_wg = kRowRoots * row_waves; o.threads = 64 * row_waves; o.lds = lds_row_each(o.roots_per_wg); break;
    case UF_ROW_SHARED:   // (the wavefronts of a workgroup that plan; the workgroup's other waves help stage the model)
        o.lanes = rowsh_rpw; o.waves = rowsh_waves; o.roots_per_wg = rowsh_rpw * rowsh_waves; o.lds = lds_row_shared(o.roots_per_wg);
        break;
    case UF_CARTPOLE: {
        // CartPole (round 6): a root is one lane, and a wavefront takes as long as its SLOWEST root's episodes -- rollouts end when
        // the pole falls, at very different lengths -- so a small batch is spread over more wavefronts of FEWER roots: 16 per
        // wave (4096 roots: 256 waves; 0.564 -> 0.550 ms).  Not fewer: wavefronts with 2 .. 8 active lanes run 1.6 - 3x SLOWER per
        // instruction when the whole chip is busy with them (tools/exec_rate.hip: an f64 division chain 180 -> 527 cycles at 4
        // active lanes x 1024 waves, unchanged at 16 or 64 lanes or on a single wave; the kernel itself 0.56 -> 1.16 ms at 4 roots
        // per wave although each wave then executes a third fewer instructions: profiles/r06_cartpole.md).
        if (k.lanes == kUnset)
            for (o.lanes = 1; o.lanes < (n + 4 * cus - 1) / (4 * cus) && o.lanes < 64;) o.lanes <<= 1;
        // Later in round 6: the slow mode is a matter of how many lanes are ACTIVE, not of how many roots a wave serves
        // (exec_rate.hip with strides: <= 8 active lanes anywhere in the wave are slow about every other run, >= 16 never).  So a
        // root is REPLICATED over 2^rep_shift lanes that all compute its plan -- 4 roots x 16 lanes at 4096 roots: 1024
        // wavefronts, one per SIMD, 669 rollout trips per wave instead of 891 -- and the replicas share the generator work (the
        // rollout block of uct_kernel).
        while ((o.lanes << (o.rep_shift + 1)) <= 64) ++o.rep_shift;
        if (k.cart_rep != kUnset)
            for (o.rep_shift = k.cart_rep; o.rep_shift > 0 && (o.lanes << o.rep_shift) > 64;) --o.rep_shift;
        if (o.rep_shift < 2) o.rep_shift = 0;      // (the replicated form works on quads)
        o.waves = k.cart_waves == 1 || k.cart_waves == 2 || k.cart_waves == 4 ? k.cart_waves : 4;
        // the per-lane path stack, then the sin / cos table of libm_sincos.hpp and the jump table: fewer waves per workgroup where
        // four would not fit the CU's LDS -- horizons beyond ~150; one wave reaches ~600 steps
        const size_t sincos = 8 + (size_t)MP_SINCOS_ENTRIES * sizeof(double) + jump;
        while (o.waves > 1 && tabs + o.waves * path_stack + sincos > kLdsBytes) o.waves >>= 1;
        o.lds = tabs + o.waves * path_stack + sincos;
        if (o.lds > kLdsBytes) return fail(MP_ERR_ARG, "mp_uct_plan: horizon %d / episodes %d need %zu B of LDS tables (> 64 KiB)", H, E, o.lds);
        break;
    }
    default:    // the gather forms: a path stack that does not fit 64 KB of LDS (horizon >~ 180) moves to registers + a global
                // spill array; MP_UCT_PATH=spill forces that
        o.lds = tabs + path_stack;
        if (o.lds > 64 * 1024 && !fallback && (c.pol || tabs > 64 * 1024))
            return fail(MP_ERR_ARG, "mp_uct_plan: horizon %d / episodes %d need %zu B of LDS tables (> 64 KiB)", H, E, o.lds);
        if (o.lds > 64 * 1024 || (k.path == 1 && !fallback && !c.pol)) {
            o.form = UF_GLOBAL_SPILL;
            o.lds = tabs;
        }
        break;
    }
    if (o.form != UF_LONE && o.form != UF_LONE_MW && o.form != UF_LONE_EACH && o.form != UF_ROW_EACH && o.form != UF_ROW_SHARED) {
        o.roots_per_wg = o.waves * o.lanes;   // uct_kernel: a lane per root (QD: four)
        o.threads = o.waves * 64;
    }
    if (c.pol && !c.cart && !at_known)
        return fail(MP_ERR_ARG, "mp_uct_plan_policy: |A| = %d is not in 2..8: per-state policies over more actions plan through "
                                "mp_uct_plan_stochastic_policy (it takes deterministic tables too)", A);
    *out = o;
    return MP_OK;
}

// one launch of the chosen form: the grid and workgroup of the choice, the kernel's LDS limit raised past the default 64 KiB
template <typename Kernel>
static int uct_go(Kernel kernel, const UctChoice &ch, const UctArgs &a, hipStream_t st)
{
    // (the progress words of the wave balance and the action table, in front of the tables)
    const size_t lds = ch.lds + (a.balance ? (size_t)kUctBalBytes : 0) + (a.action_table ? (size_t)kUctActBytes : 0);
    if (lds > 64 * 1024)
        MP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.n_roots + ch.roots_per_wg - 1) / ch.roots_per_wg)), dim3((unsigned)ch.threads), lds,
                       st, a);
    return MP_OK;
}

// the one-lane LDS-resident form with (ATAB) or without its action table: the instantiation for the call's visited mask and
// wave balance
template <int AT, bool ATAB>
static int uct_launch_ldsr(const UctChoice &ch, bool vm, const UctArgs &a, hipStream_t st)
{
    if constexpr (uct_mask_form(AT, ENV_TABLE_LDSR, false, false, 2, false))
        if (vm) {
            if constexpr (uct_balance_form(AT))
                if (a.balance) return uct_go(uct_kernel<AT, ENV_TABLE_LDSR, false, false, 2, false, true, true, ATAB>, ch, a, st);
            return uct_go(uct_kernel<AT, ENV_TABLE_LDSR, false, false, 2, false, false, true, ATAB>, ch, a, st);
        }
    if constexpr (uct_balance_form(AT))
        if (a.balance) return uct_go(uct_kernel<AT, ENV_TABLE_LDSR, false, false, 2, false, true, false, ATAB>, ch, a, st);
    return uct_go(uct_kernel<AT, ENV_TABLE_LDSR, false, false, 2, false, false, false, ATAB>, ch, a, st);
}

// the kernel of a form for |A| = AT (0: any |A|), in the tree layout a.tree_il
template <int AT>
static int uct_launch(const UctChoice &ch, bool listed, const UctArgs &a, hipStream_t st)
{
    const bool il2 = a.tree_il == 2;
    [[maybe_unused]] const bool vm = a.tree_stores == 3;   // (uct_trees: fresh trees of a form that keeps the visited mask, and no other plan)
    if constexpr (AT > 0) {
        switch (ch.form) {
        case UF_LDSR:
            if constexpr (uct_action_table_form(AT, ENV_TABLE_LDSR, false, false, 2, false))
                if (a.action_table) return uct_launch_ldsr<AT, true>(ch, vm, a, st);
            return uct_launch_ldsr<AT, false>(ch, vm, a, st);
        case UF_QUAD: return uct_go(uct_kernel<AT, ENV_TABLE_LDSR, false, false, 2, true>, ch, a, st);
        case UF_LONE: return uct_go(uct_lone_kernel<AT>, ch, a, st);
        case UF_LONE_MW: return uct_go(uct_lone_kernel<AT, false, true>, ch, a, st);
        case UF_LONE_EACH: return uct_go(uct_lone_kernel<AT, true>, ch, a, st);
        case UF_ROW_EACH: return uct_go(uct_row_kernel<AT>, ch, a, st);
        case UF_ROW_SHARED: return uct_go(uct_row_kernel<AT, true>, ch, a, st);
        case UF_POLICY:
            if (listed)
                return il2 ? uct_go(uct_kernel<AT, ENV_TABLE, true, true, 2>, ch, a, st) : uct_go(uct_kernel<AT, ENV_TABLE, true, true, 0>, ch, a, st);
            return il2 ? uct_go(uct_kernel<AT, ENV_TABLE, true, false, 2>, ch, a, st) : uct_go(uct_kernel<AT, ENV_TABLE, true, false, 0>, ch, a, st);
        case UF_GLOBAL:
            if constexpr (uct_mask_form(AT, ENV_TABLE, false, false, 2, false))
                if (il2 && vm) return uct_go(uct_kernel<AT, ENV_TABLE, false, false, 2, false, false, true>, ch, a, st);
            if (il2) return uct_go(uct_kernel<AT, ENV_TABLE, false, false, 2>, ch, a, st);
            break;
        case UF_GLOBAL_SPILL:
            if constexpr (uct_mask_form(AT, ENV_TABLE_SPILL, false, false, 2, false))
                if (il2 && vm) return uct_go(uct_kernel<AT, ENV_TABLE_SPILL, false, false, 2, false, false, true>, ch, a, st);
            if (il2) return uct_go(uct_kernel<AT, ENV_TABLE_SPILL, false, false, 2>, ch, a, st);
            break;
        default: break;
        }
    }
    if constexpr (AT == 2)   // (CartPole's two actions)
        if (ch.form == UF_CARTPOLE) return uct_go(uct_kernel<2, ENV_CARTPOLE>, ch, a, st);
    // root-major trees: generic |A|, and a kept CartPole tree continued by a table plan
    if (ch.form == UF_GLOBAL && !il2) return uct_go(uct_kernel<AT, ENV_TABLE>, ch, a, st);
    if (ch.form == UF_GLOBAL_SPILL && !il2) return uct_go(uct_kernel<AT, ENV_TABLE_SPILL>, ch, a, st);
    return fail(MP_ERR_ARG, "mp_uct_plan: no %s kernel for |A| = %d in tree layout %d", uct_form_name(ch.form).c_str(), a.A, a.tree_il);
}

// the kernel of a form for this |A|: the unrolled forms for 2..8 actions, the loop form beyond
static int uct_dispatch(const UctChoice &ch, bool listed, const UctArgs &a, hipStream_t st)
{
    static int (*const launch[8])(const UctChoice &, bool, const UctArgs &, hipStream_t) = {
        uct_launch<2>, uct_launch<3>, uct_launch<4>, uct_launch<5>, uct_launch<6>, uct_launch<7>, uct_launch<8>, uct_launch<0>};
    return launch[a.A >= 2 && a.A <= 8 ? a.A - 2 : 7](ch, listed, a, st);
}

// ---- the steps of a plan call, in the order uct_plan_impl takes them

static int uct_check(const mp_ctx *ctx, const UctPlan &c)
{
    const mp_model *model = c.model;
    const mp_policy *pol = c.pol;
    if (!ctx || !model || !c.root_state || !c.rng_state || (!pol && (!c.prior_p || !c.rollout_p)))
        return fail(MP_ERR_ARG, "mp_uct_plan: NULL argument");
    const bool cart = model->mode == MP_MODE_CARTPOLE;
    if (pol && !cart && pol->model == model && pol->model_serial == model->serial && pol->ctx == ctx && !pol->frec && pol->A > 8)
        return fail(MP_ERR_ARG, "mp_uct_plan_policy: |A| = %d is not in 2..8: per-state policies over more actions plan through "
                                "mp_uct_plan_stochastic_policy (it takes deterministic tables too)", pol->A);
    if (pol && (cart || pol->model != model || pol->model_serial != model->serial || pol->ctx != ctx || !pol->frec))
        return fail(MP_ERR_ARG, "mp_uct_plan_policy: the policy was not loaded for this model");
    if (model->mode != MP_MODE_DETERMINISTIC && !cart)
        return fail(MP_ERR_MODE, "mp_uct_plan: model mode %d is neither a deterministic table nor CartPole", model->mode);
    if (model->masked && !(pol && pol->listed))
        return fail(MP_ERR_ARG, "mp_uct_plan: the model restricts its action sets (mp_model_set_available): MCTS reads "
                                "availability through its policies -- plan with a policy from mp_policy_load_listed");
    if (c.n_roots < 1 || c.episodes < 0 || c.horizon < 0 || c.max_plan_len < 0)
        return fail(MP_ERR_ARG, "mp_uct_plan: bad sizes (n_roots=%d episodes=%d horizon=%d)", c.n_roots, c.episodes, c.horizon);
    if (!mem_valid(c.mem)) return fail(MP_ERR_ARG, "mp_uct_plan: unknown mem flags %d", c.mem);
    return MP_OK;
}

// div_by_const's conditions (see the rollout): every parameter a numerator is built from within [2^-50, 2^50], the divisor
// normal with a significand that is not all ones, the other denominator bounded away from zero.  MP_CART_FASTDIV=0: A/B.
static bool cart_fastdiv(const mp_cartpole_params &cq, double *inv_tm)
{
    const double tm = cq.masspole + cq.masscart;
    auto mid = [](double v) { return std::isfinite(v) && fabs(v) >= 0x1p-50 && fabs(v) <= 0x1p50; };
    uint64_t bits;
    memcpy(&bits, &tm, 8);
    const char *e = getenv("MP_CART_FASTDIV");
    if (!(mid(tm) && tm > 0 && (bits & ((1ULL << 52) - 1)) != (1ULL << 52) - 1 && mid(cq.masspole) && cq.masspole > 0 && mid(cq.length) &&
          cq.length > 0 && mid(cq.force_mag) && mid(cq.gravity) && mid(cq.tau) && cq.length * (4.0 / 3.0 - cq.masspole / tm) >= 0x1p-50 &&
          !(e && atoi(e) == 0)))
        return false;
    *inv_tm = 1.0 / tm;
    return true;
}

// the kernel arguments that the model, the policy and the tables decide; `thr`: the A thresholds of the tables (the tables'
// device addresses follow their upload)
static void uct_args_model(const UctPlan &c, int TE, const double *thr, UctArgs *out)
{
    const mp_model *model = c.model;
    const mp_policy *pol = c.pol;
    const int A = model->A;
    UctArgs &a = *out;
    a.n_roots = c.n_roots; a.S = model->S; a.A = A; a.episodes = c.episodes; a.horizon = c.horizon;
    a.table_n = TE;
    a.done_on_next = model->done_on_next; a.max_steps = model->max_steps; a.max_plan_len = c.max_plan_len;
    a.rec = model->rec; a.t16 = model->t16; a.tab = nullptr; a.act_tab = nullptr;
    a.r8 = model->r8; a.rdict = model->rdict; a.n_rdict = model->n_rdict;
    a.Sb = model->NB > 1 && model->Sb > 0 ? model->Sb : model->S;
    a.thr_valid = 0;
    for (int i = 0; i < 8; ++i) {
        a.thr_arg[i] = ~0ULL;
        if (i < A) {
            uint64_t t;
            memcpy(&t, &thr[i], sizeof(uint64_t));
            if (t < (1ULL << 53)) {
                a.thr_arg[i] = t << 11;
                if (i < A - 1) a.thr_valid = i + 1;     // (thresholds are non-decreasing: the valid ones are a prefix)
            }
        }
    }
    a.cp = model->cp; a.cp_sincos = model->cp_sincos;
    a.cp_inv_tm = 0.0;
    a.cp_fastdiv = model->mode == MP_MODE_CARTPOLE && cart_fastdiv(model->cp, &a.cp_inv_tm) ? 1 : 0;
    a.pol_prior = pol ? pol->prior : nullptr; a.pol_thr = pol ? pol->thr : nullptr; a.pol_frec = pol ? pol->frec : nullptr;
    a.pol_frec_roll = pol ? (pol->frec_roll ? pol->frec_roll : pol->frec) : nullptr;
    a.pol_stride = pol ? pol->stride : 0;
    // 16-byte records for saturated batches (see mp_policy_load)
    bool use16 = pol && pol->packed && c.n_roots > 16384;
    if (const char *rf = getenv("MP_UCT_POLICY_RECORD")) use16 = pol && pol->packed && rf[0] == 'p' ? true : (rf[0] == 'f' ? false : use16);
    if (pol && pol->listed) use16 = false; // the listed-action masks live in the fused records' flags word
    a.pol_shift = pol ? (use16 ? 43 : pol->shift) : 21;
    a.pol_sat = use16 ? 1023u : 0xffffffffu;
    a.pol_packed = use16 ? 1 : 0;
    if (use16) a.pol_frec = pol->frec16;
    a.TA = c.temperature * (double)A;
    a.temperature = c.temperature;
}

// limbs of A^n and G_n = 1 + A + ... + A^(n-1) (mod 2^128), n = 0..H, resident in WS_JUMP: the generator after n draws is
// A^n state + inc G_n
static int uct_jump_table(mp_ctx *ctx, int H, const uint32_t **jump)
{
    if (ctx->jump_entries < H + 5) {
        typedef unsigned __int128 u128;
        const u128 mult = ((u128)0x2360ED051FC65DA4ULL << 64) | 0x4385DF649FCCF645ULL;
        const int n_e = H + 5 > 64 ? H + 5 : 64;
        // (kept in the context: the upload is asynchronous on the planner's stream -- a caller that runs the planners
        // from a stream with pending waits, e.g. ShardedDevicePlan's double-buffered exchange, must not be synchronised here)
        ctx->jump_host.emplace_back((size_t)n_e * 8, 0u);
        std::vector<uint32_t> &tabj = ctx->jump_host.back();
        u128 an = 1, gn = 0;
        for (int n = 0; n < n_e; ++n) {
            for (int i = 0; i < 4; ++i) { tabj[(size_t)n * 8 + i] = (uint32_t)(an >> (32 * i)); tabj[(size_t)n * 8 + 4 + i] = (uint32_t)(gn >> (32 * i)); }
            gn = gn * mult + 1;
            an = an * mult;
        }
        uint32_t *dj = nullptr;
        ctx->jump_entries = 0;
        MP_TRY(ws_get(ctx, WS_JUMP, tabj.size(), &dj));
        MP_HIP(hipMemcpyAsync(dj, tabj.data(), tabj.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        ctx->jump_entries = n_e;
    }
    *jump = static_cast<const uint32_t *>(ctx->ws[WS_JUMP].p);
    return MP_OK;
}

// the action table of the call's thresholds (uct_action_table.hpp), kept in the context and rebuilt only when they change
static const std::vector<uint8_t> &uct_action_table_bytes(mp_ctx *ctx, const UctArgs &a)
{
    mp_ctx::UctActionTable &t = ctx->uct_act;
    const int nth = a.A - 1;
    if (t.bytes.size() != (size_t)kUctActBytes || t.nth != nth || t.thr_valid != a.thr_valid || memcmp(t.thr, a.thr_arg, sizeof(t.thr)) != 0) {
        t.bytes.resize(kUctActBytes);
        uct_action_table_fill(a.thr_arg, nth, a.thr_valid, t.bytes.data());
        t.nth = nth; t.thr_valid = a.thr_valid;
        memcpy(t.thr, a.thr_arg, sizeof(t.thr));
    }
    return t.bytes;
}

// the kernel form and its geometry (uct_choose), the kernel arguments they decide, the jump table of the forms that jump ahead
static int uct_form(mp_ctx *ctx, const UctPlan &c, bool cont, UctChoice *ch, UctArgs *a)
{
    const mp_model *model = c.model;
    UctCall call;
    call.n_roots = c.n_roots; call.episodes = c.episodes; call.horizon = c.horizon; call.A = model->A; call.S = model->S;
    call.NB = model->NB; call.Sb = model->Sb;
    call.t16 = model->t16 != nullptr; call.r8 = model->r8 != nullptr; call.n_rdict = model->n_rdict;
    call.cart = model->mode == MP_MODE_CARTPOLE; call.pol = c.pol != nullptr; call.listed = c.pol && c.pol->listed;
    call.kept_il = cont ? ctx->tree.il : -1;
    call.cus = ctx->prop.multiProcessorCount;
    const UctKnobs knobs = uct_knobs_read();
    MP_TRY(uct_choose(call, knobs, ch));
    a->tree_stores = knobs.tree_stores;   // (how uct_kernel issues its tree stores: neither the form nor its name)
    // the wave balance of the one-lane LDS-resident form: where the model leaves its 64 bytes, else the form runs unbalanced
    a->balance = knobs.balance && ch->form == UF_LDSR && ch->lanes == 64 && ch->lds + kUctBalBytes <= kLdsBytes &&
                 model->A >= 2 && model->A <= 8 && uct_balance_form(model->A) ? 1 : 0;
    // its action table: the same form with a state-independent policy (the form plans no other), where the model leaves the
    // table's bytes as well; else today's instantiation
    a->action_table = knobs.action_table && ch->form == UF_LDSR && ch->lanes == 64 && !c.pol &&
                      ch->lds + kUctBalBytes + kUctActBytes <= kLdsBytes &&
                      uct_action_table_form(model->A, ENV_TABLE_LDSR, false, false, ch->tree_il, false) ? 1 : 0;
    // the one-lane LDS-resident form tests bit 15 of a record under either terminal rule (THE LEAN TRIP): the table whose bit is
    // the model's rule.  Every other LDS form stages the next-state table and applies the rule itself.
    if (uct_term_table_form(ENV_TABLE_LDSR, false) && ch->form == UF_LDSR && !model->done_on_next) {
        if (!model->t16s) return fail(MP_ERR_ARG, "mp_uct_plan: the model has no source-rule transition table");
        a->t16 = model->t16s;
    }
    a->lanes = ch->lanes; a->waves = ch->waves; a->rep_shift = ch->rep_shift;
    a->jump = nullptr;
    const UctForm form = ch->form;
    if (form == UF_QUAD || form == UF_LONE || form == UF_LONE_MW || form == UF_LONE_EACH || form == UF_ROW_EACH || form == UF_ROW_SHARED ||
        form == UF_CARTPOLE)
        MP_TRY(uct_jump_table(ctx, c.horizon, &a->jump));
    return MP_OK;
}

// trees: fresh ones, or (step_strategy "subtree") the kept ones re-rooted into the other buffer with room for this plan's
// expansions; the per-root tree sizes (updated in place by re-rooting and planning); the spilled path stacks of the forms
// that keep their paths in registers
static int uct_trees(mp_ctx *ctx, const UctPlan &c, bool cont, const UctChoice &ch, UctArgs *a)
{
    const int n_roots = c.n_roots, A = a->A, H = c.horizon, E = c.episodes;
    long cap_use = 1 + (long)E * A;
    a->n_nodes_in = nullptr;
    if (cont) {
        cap_use = uct_kept_cap(ctx, H, E, A);
        MP_TRY(uct_reroot_now(ctx, cap_use)); // (reads the kept trees' sizes: before WS_TREE1 may grow to a larger selection)
        MP_TRY(ws_get(ctx, WS_TREE1, (size_t)n_roots, &a->n_nodes_out));
        a->tree = (UctNode *)ctx->ws[ctx->tree.buf ? WS_TREE2 : WS_TREE0].p;
        a->n_nodes_in = a->n_nodes_out;
    } else {
        MP_TRY(ws_get(ctx, WS_TREE1, (size_t)n_roots, &a->n_nodes_out));
        uct_fresh_tree(ctx, H, E, A);
        ctx->tree.il = ch.tree_il;
        MP_TRY(ws_get(ctx, WS_TREE0, (size_t)((n_roots + 63) & ~63) * tree_stride_alloc(ctx->tree.il, cap_use, A), &a->tree));
    }
    a->cap = (int)cap_use;
    a->tree_il = ctx->tree.il;
    a->path_spill = nullptr; a->spill_stride = 0;
    if (ch.form == UF_LDSR || ch.form == UF_QUAD || ch.form == UF_GLOBAL_SPILL) {
        a->spill_stride = ((long)n_roots + 63) & ~63L;
        MP_TRY(ws_get(ctx, WS_TREE4, (size_t)(H + 1) * (size_t)a->spill_stride, &a->path_spill));
    }
    ctx->tree.kind = 1; ctx->tree.n_roots = n_roots; ctx->tree.A = A; ctx->tree.cap = (int)cap_use;
    // fresh trees of a form that leaves zero nodes unstored (uct_kernel's VDEFER and VMASK, uct_virgin.hpp): the readers apply the
    // rule.  The visited mask needs a form that keeps it, fresh trees and first_child words below 2^24: any other plan runs the
    // count-1 form (tree_stores 2), as it did before there was a mask.
    const int env = ch.form == UF_LDSR ? ENV_TABLE_LDSR : (ch.form == UF_GLOBAL ? ENV_TABLE : (ch.form == UF_GLOBAL_SPILL ? ENV_TABLE_SPILL : -1));
    if (a->tree_stores == 3 && !(!cont && env >= 0 && uct_mask_form(A, env, false, false, ctx->tree.il, false) && cap_use <= kUctChildBits))
        a->tree_stores = 2;
    ctx->tree.virgin = kUctTreeWhole;
    if (!cont && env >= 0 && a->tree_stores == 3) ctx->tree.virgin = kUctTreeMasked;
    else if (!cont && env >= 0 && a->tree_stores == 2 && uct_virgin_form(A, env, false, false, ctx->tree.il, false)) ctx->tree.virgin = kUctTreeCount1;
    return MP_OK;
}

// ---- staging.  Device arrays are used in place; host arrays get device twins (no copy yet: the copies are issued per chunk).
// The generator records follow their own flag (MP_MEM_RNG_DEVICE: an mp_rng).  -> *all_pinned: every host array lies in
// mp_host_alloc memory.
static int uct_stage(mp_ctx *ctx, WaveIo *io, bool *all_pinned)
{
    *all_pinned = false;
    // Zero-copy: when EVERY array the caller hands over lives in mp_host_alloc memory (pinned and mapped into the
    // device's address space) the kernel reads the root states from and writes the results to the caller's arrays over
    // the bus, and the whole call is one launch + one synchronisation: no copy is issued at all.
    if (io->mem == MP_MEM_HOST) {
        void *alias[10];
        bool all = true;
        for (int i = 0; i < io->n; ++i) {
            const WaveIo::Item &t = io->item[i];
            alias[i] = t.host && t.mem == MP_MEM_HOST ? pinned_alias(ctx, t.host, io->bytes(t)) : t.host;
            if (t.host && !alias[i]) all = false;
        }
        *all_pinned = all;
        // Measured (262 144 roots, 13 MB of results): the kernel writing over the bus 1.52 ms; one launch + asynchronous
        // copies into the same pinned arrays 1.48 ms; two saturating chunks back to back on two streams, the first
        // chunk's results travelling under the second chunk's kernel, 1.35-1.37 ms (device-resident: 1.12).  Small batches
        // (4 096 roots: 0.349 ms zero-copy against 0.346 ms device-resident) are dominated by the calls a copy costs.
        long zc_max = 65536;
        if (const char *e = getenv("MP_ZERO_COPY_MAX")) zc_max = atol(e);
        if (all && !getenv("MP_NO_ZERO_COPY") && io->n_roots <= zc_max) {
            for (int i = 0; i < io->n; ++i) { io->item[i].host = alias[i]; io->item[i].mem = MP_MEM_DEVICE; }
            io->mem = MP_MEM_DEVICE; io->rmem = MP_MEM_DEVICE;     // from here on: device arrays (their aliases)
        }
    }
    // (device twins from the workspaces, NOT stage_out_alloc: that helper would hand back the device alias of a pinned
    // array -- the zero-copy form, decided above for the whole call -- and the chunk copies would copy it onto itself)
    for (int i = 0; i < io->n; ++i) {
        WaveIo::Item &t = io->item[i];
        void *d = t.host;
        if (t.mem == MP_MEM_HOST && t.host) MP_TRY(ws_reserve(ctx, t.slot, io->bytes(t), &d));
        t.base = static_cast<char *>(d);
    }
    return MP_OK;
}

// ---- one chunk of roots [r0, r1): copies in, the kernel, copies out (the generator records first, then the results in their
// ABI order), all on stream `s`.  A chunk is the same launch on shifted pointers (r0 is a multiple of 1024: whole wavefront
// blocks of the interleaved tree layouts and whole workgroups of every variant), so chunked and unchunked calls leave
// identical trees and results.  `a` holds the arguments of the whole batch; the table's pointers in it move to the chunk.
static int uct_run_chunk(const WaveIo &io, const UctChoice &ch, bool listed, UctArgs &a, int r0, int r1, hipStream_t s)
{
    const size_t cnt = (size_t)(r1 - r0);
    for (int i = 0; i < io.n; ++i) {
        const WaveIo::Item &t = io.item[i];
        char *d = t.base ? t.base + (size_t)r0 * t.per_root : nullptr;
        *t.dev = d;
        if ((t.dir & WaveIo::IN) && t.mem == MP_MEM_HOST && t.host)
            MP_HIP(hipMemcpyAsync(d, (const char *)t.host + (size_t)r0 * t.per_root, cnt * t.per_root, hipMemcpyHostToDevice, s));
    }
    UctArgs c = a;
    c.n_roots = r1 - r0;
    c.tree += (long)(r0 >> 6) * (long)tree_stride_alloc(a.tree_il, a.cap, a.A) * 64;
    if (c.path_spill) c.path_spill += r0;
    if (c.n_nodes_in) c.n_nodes_in += r0;
    c.n_nodes_out += r0;
#ifdef MP_WAVE_STAMPS
    // diagnostic build: MP_UCT_WAVE_STAMPS=<file> gets the stamps of the launch (overwritten per launch), read by tools/uct_wave_finish.py
    const char *stamp_file = getenv("MP_UCT_WAVE_STAMPS");
    const size_t stamp_words = (size_t)((c.n_roots + ch.roots_per_wg - 1) / ch.roots_per_wg) * (size_t)(ch.threads / 64) * kWaveStampWords;
    c.wave_stamps = nullptr;
    if (stamp_file) {
        MP_HIP(hipMalloc(&c.wave_stamps, stamp_words * 8));
        MP_HIP(hipMemsetAsync(c.wave_stamps, 0, stamp_words * 8, s));
    }
#endif
    MP_TRY(uct_dispatch(ch, listed, c, s));
#ifdef MP_WAVE_STAMPS
    if (stamp_file) {
        std::vector<unsigned long long> h(stamp_words);
        MP_HIP(hipStreamSynchronize(s));
        MP_HIP(hipMemcpy(h.data(), c.wave_stamps, stamp_words * 8, hipMemcpyDeviceToHost));
        MP_HIP(hipFree(c.wave_stamps));
        if (FILE *f = fopen(stamp_file, "wb")) {
            const unsigned long long head[2] = {(unsigned long long)(ch.threads / 64), (unsigned long long)kWaveStampWords};
            fwrite(head, 8, 2, f);
            fwrite(h.data(), 8, h.size(), f);
            fclose(f);
        }
    }
#endif
    for (int i = 0; i < io.n; ++i) {
        const WaveIo::Item &t = io.item[i];
        if ((t.dir & WaveIo::OUT) && t.mem == MP_MEM_HOST && t.host && t.per_root)
            MP_HIP(hipMemcpyAsync((char *)t.host + (size_t)r0 * t.per_root, *t.dev, cnt * t.per_root, hipMemcpyDeviceToHost, s));
    }
    return MP_OK;
}

// ---- host arrays and a big batch: chunks pipelined over side streams (H2D of chunk i+1 and D2H of chunk i-1 run
// under the kernel of chunk i, and kernels of different chunks share the chip).  Everything else: one chunk on the
// ctx stream, as ever.
// pageable arrays, measured at 262 144 roots: 65 536 x 4 streams 4.1 ms, 32 768 x 4 7.3 ms, 8 192 x 8 12.6 ms (the
// runtime stages every pageable copy); pinned arrays: two chunks that each fill the chip, see uct_stage
template <typename Chunk>
static int uct_pipeline(mp_ctx *ctx, int n_roots, bool host, bool all_pinned, Chunk run_chunk)
{
    int chunk = 65536, n_streams = 4;
    if (all_pinned) { chunk = (((n_roots + 1) / 2) + 1023) & ~1023; n_streams = 2; }
    if (const char *e = getenv("MP_PIPE_CHUNK")) chunk = atoi(e) > 0 ? ((atoi(e) + 1023) & ~1023) : 0;
    if (const char *e = getenv("MP_PIPE_STREAMS")) { const int v = atoi(e); if (v >= 1 && v <= 8) n_streams = v; }
    const bool piped = host && chunk > 0 && n_roots > chunk;
    MP_TRY(kernels_begin(ctx));
    int launches = 1;
    if (piped) {
        const int n_chunks = (n_roots + chunk - 1) / chunk;
        if (n_streams > n_chunks) n_streams = n_chunks;
        MP_TRY(pipe_fork(ctx, n_streams));
        for (int c = 0; c < n_chunks; ++c) {
            const int r0 = c * chunk, r1 = r0 + chunk < n_roots ? r0 + chunk : n_roots;
            MP_TRY(run_chunk(r0, r1, ctx->pipe[c % n_streams]));
        }
        MP_TRY(pipe_join(ctx, n_streams));
        launches = n_chunks;
    } else {
        MP_TRY(run_chunk(0, n_roots, ctx->stream));
    }
    MP_TRY(kernels_end(ctx, launches));
    MP_HIP(hipGetLastError());
    return MP_OK;
}

static int uct_plan_impl(mp_ctx *ctx, const UctPlan &c)
{
    MP_TRY(uct_check(ctx, c));
    mp_model *model = c.model;
    const bool cart = model->mode == MP_MODE_CARTPOLE;
    const int n_roots = c.n_roots, A = model->A, H = c.horizon, E = c.episodes;
    MP_HIP(hipSetDevice(ctx->device));

    // small per-call tables
    // (the quotient tables live in LDS: 16 KB of them at most; counts beyond take the division in the kernel)
    const int te_max = (int)(16384 / (sizeof(double) * (size_t)(A + 1)));
    const int TE = E < te_max ? E : te_max;
    std::vector<double> tab;
    const UctTables to = uct_tables(H, A, TE, c.gamma, c.temperature, c.prior_p, c.rollout_p, tab);

    UctArgs a;
    uct_args_model(c, TE, tab.data() + to.cdf, &a);
    // the kernel form and its geometry: nothing below changes them
    const bool cont = ctx->tree.armed && ctx->tree.kind == 1 && ctx->tree.n_roots == n_roots && ctx->tree.A == A;
    UctChoice ch;
    MP_TRY(uct_form(ctx, c, cont, &ch, &a));
    // the tables go up in one block, the action table of a launch that takes it behind the others (16-byte aligned): one copy on
    // the planner's stream, and none while the block is what the last call uploaded
    const size_t act_at = (to.n + 1) & ~(size_t)1;
    if (a.action_table) {
        const std::vector<uint8_t> &bytes = uct_action_table_bytes(ctx, a);
        tab.resize(act_at + kUctActBytes / sizeof(double), 0.0);
        memcpy(tab.data() + act_at, bytes.data(), kUctActBytes);
    }
    double *d_tab = nullptr;
    MP_TRY(upload_tables(ctx, 1, tab, &d_tab));
    a.tab = d_tab;
    a.act_tab = a.action_table ? reinterpret_cast<const uint8_t *>(d_tab + act_at) : nullptr;
    MP_TRY(uct_trees(ctx, c, cont, ch, &a));
    form_record(ctx->last_variant, uct_form_name(ch.form));
    ctx->uct_action_table = a.action_table;

    // the caller's arrays: root states, steps and generator records in, the records and the results out
    const bool host_call = mem_arrays(c.mem) == MP_MEM_HOST;       // the call synchronises before it returns
    WaveIo io(mem_arrays(c.mem), mem_rng(c.mem), n_roots);
    a.root_x = nullptr; a.root_state = nullptr;
    if (cart) io.in(WS_IO9, (const double *)c.root_state, &a.root_x, 4);
    else io.in(WS_IO0, (const int32_t *)c.root_state, &a.root_state);
    io.in(WS_IO1, c.root_steps, &a.root_steps);
    io.rng(c.rng_state, &a.rng);
    io.add(WS_IO3, c.plans, &a.plans, c.max_plan_len);
    io.add(WS_IO4, c.plan_len, &a.plan_len);
    io.add(WS_IO5, c.root_value, &a.root_value);
    io.add(WS_IO6, c.root_child_count, &a.root_child_count, A);
    io.add(WS_IO7, c.root_child_value, &a.root_child_value, A);
    io.add(WS_IO8, c.env_steps, &a.env_steps);
    bool all_pinned = false;
    MP_TRY(uct_stage(ctx, &io, &all_pinned));

    const bool listed = c.pol && c.pol->listed;
    MP_TRY(uct_pipeline(ctx, n_roots, io.mem == MP_MEM_HOST, all_pinned,
                        [&](int r0, int r1, hipStream_t s) { return uct_run_chunk(io, ch, listed, a, r0, r1, s); }));
    if (host_call) MP_HIP(hipStreamSynchronize(ctx->stream));
    return MP_OK;
}

extern "C" {

int mp_uct_plan(mp_ctx *ctx, mp_model *model, int32_t n_roots, const void *root_state, const int32_t *root_steps,
                int32_t episodes, int32_t horizon, double gamma, double temperature, const double *prior_p,
                const double *rollout_p, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                int32_t *plan_len, double *root_value, int64_t *root_child_count, double *root_child_value,
                int64_t *env_steps, int32_t mem)
{
    return uct_plan_impl(ctx, {model, nullptr, n_roots, root_state, root_steps, episodes, horizon, gamma, temperature, prior_p,
                               rollout_p, 0, rng_state, nullptr, max_plan_len, plans, plan_len, root_value, root_child_count,
                               root_child_value, env_steps, mem});
}

int mp_uct_plan_models(mp_ctx *ctx, mp_model *model, int32_t n_roots, const int32_t *model_index, const int32_t *root_state,
                       const int32_t *root_steps, int32_t episodes, int32_t horizon, double gamma, double temperature,
                       const double *prior_p, const double *rollout_p, uint64_t *rng_state, int32_t max_plan_len, int32_t *plans,
                       int32_t *plan_len, double *root_value, int64_t *root_child_count, double *root_child_value,
                       int64_t *env_steps, int32_t mem)
{
    if (!mem_valid(mem)) return fail(MP_ERR_ARG, "mp_uct_plan_models: unknown mem flags %d", mem);
    std::vector<int32_t> tmp;
    const int32_t *global = nullptr;
    MP_TRY(globalize_roots_arg(ctx, model, n_roots, model_index, root_state, mem, tmp, &global));
    return uct_plan_impl(ctx, {model, nullptr, n_roots, global, root_steps, episodes, horizon, gamma, temperature, prior_p,
                               rollout_p, 0, rng_state, nullptr, max_plan_len, plans, plan_len, root_value, root_child_count,
                               root_child_value, env_steps, mem});
}

int mp_uct_plan_policy(mp_ctx *ctx, mp_model *model, mp_policy *policy, int32_t n_roots, const void *root_state,
                       const int32_t *root_steps, int32_t episodes, int32_t horizon, double gamma, double temperature,
                       uint64_t *rng_state, int32_t max_plan_len, int32_t *plans, int32_t *plan_len, double *root_value,
                       int64_t *root_child_count, double *root_child_value, int64_t *env_steps, int32_t mem)
{
    if (!policy) return fail(MP_ERR_ARG, "mp_uct_plan_policy: policy is NULL");
    return uct_plan_impl(ctx, {model, policy, n_roots, root_state, root_steps, episodes, horizon, gamma, temperature, nullptr,
                               nullptr, 0, rng_state, nullptr, max_plan_len, plans, plan_len, root_value, root_child_count,
                               root_child_value, env_steps, mem});
}

int mp_uct_last_action_table(mp_ctx *ctx) { return ctx ? ctx->uct_action_table : 0; }

// mcts_with_prior.py:47-62 as tables: per state, the prior row and the integer sampling thresholds of the rollout row
// (computed exactly as mp_uct_plan computes them for one distribution), plus one fused record per (s, a).
int mp_uct_choose_form(const int64_t *call, int64_t *out, const char **name)
{
    if (!call || !out || !name) return fail(MP_ERR_ARG, "mp_uct_choose_form: NULL argument");
    UctCall c;
    c.n_roots = (int)call[0]; c.episodes = (int)call[1]; c.horizon = (int)call[2]; c.A = (int)call[3]; c.S = (int)call[4];
    c.NB = (int)call[5]; c.Sb = (int)call[6]; c.t16 = call[7] != 0; c.r8 = call[8] != 0; c.n_rdict = (int)call[9];
    c.cart = call[10] != 0; c.pol = call[11] != 0; c.listed = call[11] == 2; c.kept_il = (int)call[12]; c.cus = (int)call[13];
    UctChoice ch;
    MP_TRY(uct_choose(c, uct_knobs_read(), &ch));
    out[0] = ch.tree_il; out[1] = ch.lanes; out[2] = ch.waves; out[3] = ch.rep_shift; out[4] = ch.roots_per_wg; out[5] = ch.threads;
    out[6] = (int64_t)ch.lds;
    *name = uct_form_name_static(ch.form);
    return MP_OK;
}

int mp_policy_load(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout, mp_policy **out)
{
    return mp_policy_load_listed(ctx, model, prior, rollout, nullptr, out);
}

int mp_policy_load_listed(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout, const uint8_t *listed,
                          mp_policy **out)
{
    return mp_policy_load_ordered(ctx, model, prior, rollout, listed, nullptr, out);
}

// rollout_slot (uint8 [S][A], nullptr = identity): the order in which the ROLLOUT policy lists the actions of a state --
// slot k of state s is column rollout_slot[s][k] (a permutation of the columns; zero-probability columns last).  The
// rollout's inverse CDF runs over slots, so the tree (columns: the PRIOR policy's listing order, which decides child
// order and tie-breaks) and the rollout may list the actions differently: policy type `random` lists np.arange(n)
// whatever the environment lists (mcts.py:46-57).  A rollout step never touches the tree -- it needs the next state,
// the reward, the flags and the next state's thresholds -- so its fused records are simply laid out by slot.
int mp_policy_load_ordered(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout, const uint8_t *listed,
                           const uint8_t *rollout_slot, mp_policy **out)
{
    return mp_policy_load_rows(ctx, model, prior, rollout, listed, rollout_slot, model ? model->S : 0, out);
}

// The fused policy built by kernels (see PolBuild).  One block from the ctx's block cache holds every array.
static int policy_build_device(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout, const uint8_t *listed,
                               const uint8_t *rollout_slot, int rows, mp_policy **out)
{
    const int S = model->S, A = model->A;
    const int stride = (A + 1) & ~1, frq = 1 + (A - 1 + 3) / 4;
    int shift = 21;
    if (const char *e = getenv("MP_UCT_COARSE_BITS")) {
        const int n = atoi(e);
        if (n >= 1 && n <= 32) shift = 53 - n;
    }
    const bool can_pack = A <= 5 && S <= (1 << 20) && !getenv("MP_UCT_COARSE_BITS") && !listed && !rollout_slot;
    hipStream_t st = ctx->stream;
    // inputs -> workspace
    double *d_prior = nullptr, *d_roll = nullptr;
    uint8_t *d_listed = nullptr, *d_slot = nullptr;
    int32_t *d_err = nullptr;
    const size_t nin = (size_t)rows * A;
    MP_TRY(ws_get(ctx, WS_POL0, nin, &d_prior));
    MP_TRY(ws_get(ctx, WS_POL1, nin, &d_roll));
    MP_TRY(ws_get(ctx, WS_POL4, 2, &d_err));
    MP_HIP(hipMemcpyAsync(d_prior, prior, nin * 8, hipMemcpyHostToDevice, st));
    if (rollout == prior) d_roll = d_prior;
    else MP_HIP(hipMemcpyAsync(d_roll, rollout, nin * 8, hipMemcpyHostToDevice, st));
    if (listed) {
        MP_TRY(ws_get(ctx, WS_POL2, nin, &d_listed));
        MP_HIP(hipMemcpyAsync(d_listed, listed, nin, hipMemcpyHostToDevice, st));
    }
    if (rollout_slot) {
        MP_TRY(ws_get(ctx, WS_POL3, nin, &d_slot));
        MP_HIP(hipMemcpyAsync(d_slot, rollout_slot, nin, hipMemcpyHostToDevice, st));
    }
    MP_HIP(hipMemsetAsync(d_err, 0, 8, st));
    // outputs: one block
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_hp = al((size_t)S * stride * 8), b_ht = b_hp, b_hf = al((size_t)S * A * frq * 16), b_lm = al((size_t)S * 4),
                 b_hfr = rollout_slot ? b_hf : 0, b_p16 = can_pack ? al((size_t)S * A * 16) : 0, b_rs = rollout_slot ? al((size_t)S * A) : 0;
    mp_policy *pol = new (std::nothrow) mp_policy;
    if (!pol) return fail(MP_ERR_ALLOC, "mp_policy_load: out of memory");
    pol->ctx = ctx; pol->model = model; pol->model_serial = model->serial; pol->S = S; pol->A = A; pol->stride = stride; pol->frq = frq;
    pol->shift = shift; pol->packed = can_pack ? 1 : 0; pol->listed = listed ? 1 : 0;
    size_t got = 0;
    if (ctx_block_alloc(ctx, &pol->block, b_hp + b_ht + b_hf + b_lm + b_hfr + b_p16 + b_rs, &got) != hipSuccess) {
        (void)hipGetLastError();
        delete pol;
        return fail(MP_ERR_ALLOC, "mp_policy_load: device allocation failed");
    }
    pol->block_bytes = got;
    char *base = static_cast<char *>(pol->block);
    pol->prior = reinterpret_cast<double *>(base); base += b_hp;
    pol->thr = reinterpret_cast<uint64_t *>(base); base += b_ht;
    pol->frec = reinterpret_cast<uint4 *>(base); base += b_hf;
    pol->lmask = reinterpret_cast<uint32_t *>(base); base += b_lm;
    if (rollout_slot) { pol->frec_roll = reinterpret_cast<uint4 *>(base); base += b_hfr; }
    if (can_pack) { pol->frec16 = reinterpret_cast<uint4 *>(base); base += b_p16; }
    if (rollout_slot) { pol->rslot = reinterpret_cast<uint8_t *>(base); base += b_rs; }
    PolBuild b;
    b.S = S; b.A = A; b.stride = stride; b.frq = frq; b.rows = rows; b.shift = shift; b.can_pack = can_pack ? 1 : 0;
    b.prior = d_prior; b.rollout = d_roll; b.listed = d_listed; b.slot = d_slot; b.rec = model->rec;
    b.hp = pol->prior; b.ht = pol->thr; b.lmask = pol->lmask; b.hf = reinterpret_cast<uint32_t *>(pol->frec);
    b.hfr = reinterpret_cast<uint32_t *>(pol->frec_roll); b.hp16 = reinterpret_cast<uint32_t *>(pol->frec16); b.err = d_err;
    hipLaunchKernelGGL(policy_rows_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, b);
    hipLaunchKernelGGL(policy_frec_kernel, dim3((unsigned)(((size_t)S * A + 255) / 256)), dim3(256), 0, st, b);
    if (rollout_slot) {
        hipLaunchKernelGGL(policy_froll_kernel, dim3((unsigned)(((size_t)S * A + 255) / 256)), dim3(256), 0, st, b);
        // the slots' columns by GLOBAL state (uct_stoch.hip reads them): tile the rows
        for (int off = 0; off < S; off += rows)
            MP_HIP(hipMemcpyAsync(pol->rslot + (size_t)off * A, d_slot, (size_t)(S - off < rows ? S - off : rows) * A, hipMemcpyDeviceToDevice, st));
    }
    int32_t err[2] = {0, 0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(err, d_err, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        mp_policy_free(pol);
        return fail(MP_ERR_HIP, "mp_policy_load: %s", hipGetErrorString(e));
    }
    if (err[0]) {
        mp_policy_free(pol);
        const int s_bad = err[1];
        switch (err[0]) {
        case 1: return fail(MP_ERR_ARG, "mp_policy_load: negative or NaN probability in state %d", s_bad);
        case 2: return fail(MP_ERR_ARG, "mp_policy_load: rollout distribution of state %d sums to 0", s_bad);
        case 3: return fail(MP_ERR_ARG, "mp_policy_load_listed: the prior policy lists no action in state %d", s_bad);
        case 4: return fail(MP_ERR_ARG, "mp_policy_load_ordered: rollout_slot of state %d is not a permutation", s_bad);
        default: return fail(MP_ERR_ARG, "mp_policy_load: transition out of range");
        }
    }
    *out = pol;
    return MP_OK;
}

// `rows` = S: one distribution row per state of the model; `rows` = the states of ONE MDP of a batch model
// (mp_model_load_table_batch): the rows are given for local states and serve every MDP of the batch.
int mp_policy_load_rows(mp_ctx *ctx, mp_model *model, const double *prior, const double *rollout, const uint8_t *listed,
                        const uint8_t *rollout_slot, int32_t rows, mp_policy **out)
{
    if (!ctx || !model || !prior || !rollout || !out) return fail(MP_ERR_ARG, "mp_policy_load: NULL argument");
    if (rows != model->S && !(model->NB > 1 && model->Sb > 0 && rows == model->Sb))
        return fail(MP_ERR_ARG, "mp_policy_load_rows: %d rows for a model of %d states (%d MDPs of %d)", rows, model->S, model->NB, model->Sb);
    {
        const bool det = model->mode == MP_MODE_DETERMINISTIC && model->rec && model->A >= 2 && model->A <= 8;
        const char *how = getenv("MP_POLICY_BUILD"); // "host" / "device": test knob
        const bool big = (size_t)model->S * model->A >= 16384;
        if (det && (rows != model->S || (how ? how[0] == 'd' : big))) {
            MP_HIP(hipSetDevice(ctx->device));
            return policy_build_device(ctx, model, prior, rollout, listed, rollout_slot, rows, out);
        }
        if (rows != model->S) return fail(MP_ERR_ARG, "mp_policy_load_rows: tiled rows need a deterministic table model with 2..8 actions");
    }
    const bool stoch = model->mode == MP_MODE_STOCHASTIC || model->mode == MP_MODE_SPARSE; // policies for uct_stoch.hip
    if (!stoch && (model->mode != MP_MODE_DETERMINISTIC || !model->rec))
        return fail(MP_ERR_MODE, "mp_policy_load: per-state policies need a finite-MDP model");
    const int S = model->S, A = model->A;
    if (A < 2) return fail(MP_ERR_ARG, "mp_policy_load: |A| = %d", A);
    if (rollout_slot && A > 256) return fail(MP_ERR_ARG, "mp_policy_load_ordered: rollout slots hold a byte per column (|A| = %d > 256)", A);
    // More than 8 actions (round 4): the policy of the loop-form kernel (uct_stoch.hip plans on deterministic tables too): priors,
    // thresholds, listed actions -- no fused records, whatever the model's mode
    const bool loop_form = stoch || A > 8;
    MP_HIP(hipSetDevice(ctx->device));
    const int stride = (A + 1) & ~1, frq = 1 + (A - 1 + 3) / 4;
    std::vector<double> hp((size_t)S * stride, 0.0);
    std::vector<uint64_t> ht((size_t)S * stride, ~0ULL);
    // column of slot k in state s
    auto col = [&](int s, int k) { return rollout_slot ? (int)rollout_slot[(size_t)s * A + k] : k; };
    if (rollout_slot)
        for (int s = 0; s < S; ++s) {
            std::vector<uint8_t> seen((size_t)A, 0);
            for (int k = 0; k < A; ++k) {
                const int c = rollout_slot[(size_t)s * A + k];
                if (c >= A || seen[(size_t)c]) return fail(MP_ERR_ARG, "mp_policy_load_ordered: rollout_slot of state %d is not a permutation", s);
                seen[(size_t)c] = 1;
            }
        }
    for (int s = 0; s < S; ++s) {
        std::vector<double> cdf((size_t)A);
        double acc = 0.0;
        for (int a = 0; a < A; ++a) {
            const double q = rollout[(size_t)s * A + col(s, a)], pr = prior[(size_t)s * A + a];
            if (!(q >= 0.0) || !(pr >= 0.0)) return fail(MP_ERR_ARG, "mp_policy_load: negative or NaN probability in state %d", s);
            hp[(size_t)s * stride + a] = pr;
            acc += q; cdf[a] = acc;                                                // numpy cumsum, in the rollout policy's order
        }
        if (!(acc > 0.0)) return fail(MP_ERR_ARG, "mp_policy_load: rollout distribution of state %d sums to 0", s);
        for (int a = 0; a < A; ++a) {
            const double scaled = ceil(ldexp(cdf[a] / acc, 53));                   // cdf /= cdf[-1]; see mp_uct_plan
            ht[(size_t)s * stride + a] = scaled >= 18446744073709551615.0 ? ~0ULL : (uint64_t)scaled;
        }
    }
    if (loop_form) {
        // a stochastic model's kernel stores priors in the tree and reads thresholds by state: prior / thresholds / listed
        // masks (+ the rollout slots' columns) are all it needs -- no fused records
        std::vector<uint32_t> lm((size_t)S, A >= 32 ? 0xffffffffu : (1u << A) - 1u);
        std::vector<uint8_t> l8(A > 32 ? (size_t)S * A : 0, 1); // more than 32 actions: a byte per action
        if (listed)
            for (int s = 0; s < S; ++s) {
                uint32_t m = 0;
                bool any = false;
                for (int a = 0; a < A; ++a) {
                    const bool on = listed[(size_t)s * A + a] != 0;
                    any |= on;
                    if (a < 32) m |= (on ? 1u : 0u) << a;
                    if (A > 32) l8[(size_t)s * A + a] = on ? 1 : 0;
                }
                if (!any) return fail(MP_ERR_ARG, "mp_policy_load_listed: the prior policy lists no action in state %d", s);
                lm[(size_t)s] = m;
            }
        mp_policy *pol = new (std::nothrow) mp_policy;
        if (!pol) return fail(MP_ERR_ALLOC, "mp_policy_load: out of memory");
        pol->ctx = ctx; pol->model = model; pol->model_serial = model->serial; pol->S = S; pol->A = A; pol->stride = stride;
        pol->listed = listed ? 1 : 0;
        if (hipMalloc(&pol->prior, hp.size() * 8) != hipSuccess || hipMalloc(&pol->thr, ht.size() * 8) != hipSuccess ||
            hipMalloc(&pol->lmask, lm.size() * 4) != hipSuccess ||
            (!l8.empty() && hipMalloc(&pol->listed8, l8.size()) != hipSuccess) ||
            (rollout_slot && hipMalloc(&pol->rslot, (size_t)S * A) != hipSuccess)) {
            mp_policy_free(pol);
            return fail(MP_ERR_ALLOC, "mp_policy_load: device allocation failed");
        }
        MP_HIP(hipMemcpy(pol->prior, hp.data(), hp.size() * 8, hipMemcpyHostToDevice));
        MP_HIP(hipMemcpy(pol->thr, ht.data(), ht.size() * 8, hipMemcpyHostToDevice));
        MP_HIP(hipMemcpy(pol->lmask, lm.data(), lm.size() * 4, hipMemcpyHostToDevice));
        if (!l8.empty()) MP_HIP(hipMemcpy(pol->listed8, l8.data(), l8.size(), hipMemcpyHostToDevice));
        if (rollout_slot) MP_HIP(hipMemcpy(pol->rslot, rollout_slot, (size_t)S * A, hipMemcpyHostToDevice));
        *out = pol;
        return MP_OK;
    }
    std::vector<Rec> hrec((size_t)S * A);
    MP_HIP(hipStreamSynchronize(ctx->stream));
    MP_HIP(hipMemcpy(hrec.data(), model->rec, hrec.size() * sizeof(Rec), hipMemcpyDeviceToHost));
    // MP_UCT_COARSE_BITS=n (1..32, default 32): keep only the top n bits in the fused records -- a test knob that
    // makes the exact-row fallback frequent (probability ~|A| * 2^-n per step)
    int shift = 21;
    if (const char *e = getenv("MP_UCT_COARSE_BITS")) {
        const int n = atoi(e);
        if (n >= 1 && n <= 32) shift = 53 - n;
    }
    // record formats: always 32 / 48 bytes with 32 coarse bits per threshold; when |A| <= 5 and S <= 2^20 also 16 bytes
    // (10 coarse bits per threshold in the spare bits of next and flags), which saturated batches use (one gather per
    // rollout step instead of two: +5-9 % there, -5 % on a lone wave).  MP_UCT_POLICY_RECORD=fused / packed forces one.
    const bool can_pack = A <= 5 && S <= (1 << 20) && !getenv("MP_UCT_COARSE_BITS") && !listed && !rollout_slot;
    std::vector<uint32_t> lmask((size_t)S, (1u << A) - 1u); // actions the prior policy lists per state
    if (listed)
        for (int s = 0; s < S; ++s) {
            uint32_t m = 0;
            for (int a = 0; a < A; ++a) m |= (listed[(size_t)s * A + a] ? 1u : 0u) << a;
            if (!m) return fail(MP_ERR_ARG, "mp_policy_load_listed: the prior policy lists no action in state %d", s);
            lmask[(size_t)s] = m;
        }
    std::vector<uint32_t> hf((size_t)S * A * frq * 4, 0xffffffffu), hp16(can_pack ? (size_t)S * A * 4 : 0);
    for (size_t i = 0; i < (size_t)S * A; ++i) {
        uint32_t *f = hf.data() + i * frq * 4;
        memcpy(f, &hrec[i], sizeof(Rec));
        const int nx = hrec[i].next;
        if (nx < 0 || nx >= S) return fail(MP_ERR_ARG, "mp_policy_load: transition out of range");
        f[1] = (hrec[i].flags & 0xffu) | (lmask[(size_t)nx] << 8) | (lmask[i / (size_t)A] << 16);
        uint32_t th[4] = {1023u, 1023u, 1023u, 1023u};
        for (int a = 0; a + 1 < A; ++a) {
            const uint64_t t53 = ht[(size_t)nx * stride + a];
            const uint64_t hi = t53 >> shift;                                      // top bits of the 53, saturated
            f[4 + a] = hi > 0xffffffffULL ? 0xffffffffu : (uint32_t)hi;
            if (can_pack) th[a] = (t53 >> 43) > 1023ULL ? 1023u : (uint32_t)(t53 >> 43);
        }
        if (can_pack) {
            uint32_t *g = hp16.data() + i * 4;
            memcpy(g, &hrec[i], sizeof(Rec));
            g[0] = (uint32_t)nx | (th[0] << 20);
            g[1] = (hrec[i].flags & 3u) | (th[1] << 2) | (th[2] << 12) | (th[3] << 22);
        }
    }
    // records of the rollout, by slot: entry (s, k) = the record of (s, column of slot k) + the next state's thresholds
    std::vector<uint32_t> hfr;
    if (rollout_slot) {
        hfr.resize(hf.size());
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < A; ++k)
                memcpy(hfr.data() + ((size_t)s * A + k) * frq * 4, hf.data() + ((size_t)s * A + col(s, k)) * frq * 4, (size_t)frq * 16);
    }
    mp_policy *pol = new (std::nothrow) mp_policy;
    if (!pol) return fail(MP_ERR_ALLOC, "mp_policy_load: out of memory");
    pol->ctx = ctx; pol->model = model; pol->model_serial = model->serial; pol->S = S; pol->A = A; pol->stride = stride; pol->frq = frq; pol->shift = shift; pol->packed = can_pack ? 1 : 0; pol->listed = listed ? 1 : 0;
    if (hipMalloc(&pol->prior, hp.size() * 8) != hipSuccess || hipMalloc(&pol->thr, ht.size() * 8) != hipSuccess ||
        hipMalloc(&pol->frec, hf.size() * 4) != hipSuccess || hipMalloc(&pol->lmask, lmask.size() * 4) != hipSuccess ||
        (rollout_slot && hipMalloc(&pol->rslot, (size_t)S * A) != hipSuccess) ||
        (rollout_slot && hipMalloc(&pol->frec_roll, hfr.size() * 4) != hipSuccess) ||
        (can_pack && hipMalloc(&pol->frec16, hp16.size() * 4) != hipSuccess)) {
        mp_policy_free(pol);
        return fail(MP_ERR_ALLOC, "mp_policy_load: device allocation failed");
    }
    MP_HIP(hipMemcpy(pol->prior, hp.data(), hp.size() * 8, hipMemcpyHostToDevice));
    MP_HIP(hipMemcpy(pol->thr, ht.data(), ht.size() * 8, hipMemcpyHostToDevice));
    MP_HIP(hipMemcpy(pol->frec, hf.data(), hf.size() * 4, hipMemcpyHostToDevice));
    // (the same policy also plans through mp_uct_plan_stochastic_policy -- which takes deterministic tables -- e.g. when a
    // binding replays a plan with the visit counter armed: that kernel reads the listed masks and the rollout slots' columns)
    MP_HIP(hipMemcpy(pol->lmask, lmask.data(), lmask.size() * 4, hipMemcpyHostToDevice));
    if (rollout_slot) MP_HIP(hipMemcpy(pol->rslot, rollout_slot, (size_t)S * A, hipMemcpyHostToDevice));
    if (can_pack) MP_HIP(hipMemcpy(pol->frec16, hp16.data(), hp16.size() * 4, hipMemcpyHostToDevice));
    if (rollout_slot) MP_HIP(hipMemcpy(pol->frec_roll, hfr.data(), hfr.size() * 4, hipMemcpyHostToDevice));
    *out = pol;
    return MP_OK;
}

int mp_policy_free(mp_policy *policy)
{
    if (!policy) return MP_OK;
    if (policy->block) { // built on the device: one block of the ctx's cache holds every array
        ctx_block_release(policy->ctx, policy->block, policy->block_bytes);
        delete policy;
        return MP_OK;
    }
    if (policy->prior) (void)hipFree(policy->prior);
    if (policy->thr) (void)hipFree(policy->thr);
    if (policy->frec) (void)hipFree(policy->frec);
    if (policy->frec16) (void)hipFree(policy->frec16);
    if (policy->frec_roll) (void)hipFree(policy->frec_roll);
    if (policy->lmask) (void)hipFree(policy->lmask);
    if (policy->rslot) (void)hipFree(policy->rslot);
    if (policy->listed8) (void)hipFree(policy->listed8);
    delete policy;
    return MP_OK;
}

// mp_uct_step_tree (source == nullptr: root i continues root i) and mp_uct_step_tree_select
static int uct_step_tree_impl(mp_ctx *ctx, const char *who, int32_t n_new, const int32_t *source, const int32_t *actions, int32_t mem)
{
    if (!ctx || !actions) return fail(MP_ERR_ARG, "%s: NULL argument", who);
    const bool stoch = ctx->tree.kind == 4 && ctx->tree.K == 0; // open-loop trees of mp_uct_plan_stochastic
    if ((ctx->tree.kind != 1 && !stoch) || (!source && ctx->tree.n_roots != n_new))
        return fail(MP_ERR_ARG, "%s: no UCT trees of %d roots on this ctx (closed-loop trees cannot be re-used)", who, n_new);
    if (n_new < 1) return fail(MP_ERR_ARG, "%s: %d roots", who, n_new);
    const int n_old = ctx->tree.n_roots; // (with a selection pending: the roots IT selects, which the new one counts from)
    if (source && mem == MP_MEM_HOST)
        for (int i = 0; i < n_new; ++i)
            if (source[i] < 0 || source[i] >= n_old)
                return fail(MP_ERR_ARG, "%s: source_root[%d] = %d is not one of the %d roots of the last plan", who, i, source[i], n_old);
    MP_HIP(hipSetDevice(ctx->device));
    // (room for this call's arrays first, keeping what a pending step left there: once the pending re-rooting below has run the
    // trees have moved a level, and nothing after it may fail for want of memory)
    MP_TRY(ws_reserve_keep(ctx, WS_TREE3, (size_t)n_new * sizeof(int32_t)));
    if (source) MP_TRY(ws_reserve_keep(ctx, WS_TREE7, (size_t)2 * n_new * sizeof(int32_t)));
    // a second step before the next plan (receding_horizon > 1: abstract.py:70-82 steps the tree on every act) descends
    // one more level: apply the pending re-rooting now, then arm the new one
    if (ctx->tree.armed) MP_TRY(stoch ? uct_stoch_reroot_now(ctx, ctx->tree.cap) : uct_reroot_now(ctx, ctx->tree.cap));
    const hipMemcpyKind kind = mem == MP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    int32_t *d = nullptr;
    MP_TRY(ws_get(ctx, WS_TREE3, (size_t)n_new, &d));
    MP_HIP(hipMemcpyAsync(d, actions, (size_t)n_new * sizeof(int32_t), kind, ctx->stream));
    if (source) { // [n_new] sources, then room for the [n_new] sizes the re-rooting writes
        int32_t *ds = nullptr;
        MP_TRY(ws_get(ctx, WS_TREE7, (size_t)2 * n_new, &ds));
        MP_HIP(hipMemcpyAsync(ds, source, (size_t)n_new * sizeof(int32_t), kind, ctx->stream));
    }
    if (mem == MP_MEM_HOST) MP_HIP(hipStreamSynchronize(ctx->stream));
    ctx->tree.n_src = source ? n_old : 0;
    ctx->tree.n_roots = n_new;
    ctx->tree.armed = true;
    return MP_OK;
}

int mp_uct_step_tree(mp_ctx *ctx, int32_t n_roots, const int32_t *actions, int32_t mem)
{
    return uct_step_tree_impl(ctx, "mp_uct_step_tree", n_roots, nullptr, actions, mem);
}

int mp_uct_step_tree_select(mp_ctx *ctx, int32_t n_new, const int32_t *source_root, const int32_t *actions, int32_t mem)
{
    if (!source_root) return fail(MP_ERR_ARG, "mp_uct_step_tree_select: NULL argument");
    return uct_step_tree_impl(ctx, "mp_uct_step_tree_select", n_new, source_root, actions, mem);
}

int mp_uct_tree_capacity(mp_ctx *ctx, int32_t *cap)
{
    if (!ctx || !cap) return fail(MP_ERR_ARG, "mp_uct_tree_capacity: NULL argument");
    if (ctx->tree.kind != 1) return fail(MP_ERR_ARG, "mp_uct_tree_capacity: no UCT tree on this ctx");
    *cap = ctx->tree.cap;
    return MP_OK;
}

int mp_uct_reset_tree(mp_ctx *ctx)
{
    if (!ctx) return fail(MP_ERR_ARG, "ctx is NULL");
    // (a selection that is dropped: the trees are the last plan's; every planner that replaces them clears n_src)
    if (selection_pending(ctx)) ctx->tree.n_roots = ctx->tree.n_src;
    ctx->tree.armed = false;
    ctx->tree.n_src = 0;
    return MP_OK;
}

int mp_uct_path_count(mp_ctx *ctx, int32_t root, const int32_t *actions, int32_t n, int64_t *count)
{
    if (!ctx || !count || (n > 0 && !actions)) return fail(MP_ERR_ARG, "mp_uct_path_count: NULL argument");
    if (ctx->tree.kind != 1) return fail(MP_ERR_ARG, "mp_uct_path_count: no UCT tree on this ctx");
    if (root < 0 || root >= ctx->tree.n_roots || n < 0) return fail(MP_ERR_ARG, "mp_uct_path_count: root %d / length %d out of range", root, n);
    if (selection_pending(ctx)) return fail(MP_ERR_ARG, "mp_uct_path_count: a selection of the trees is armed: plan (or mp_uct_reset_tree) first");
    MP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    UctNode *trees = (UctNode *)ctx->ws[ctx->tree.buf ? WS_TREE2 : WS_TREE0].p;
    int32_t *d_act = nullptr;
    int64_t *d_out = nullptr;
    MP_TRY(ws_get(ctx, WS_IO1, (size_t)(n > 0 ? n : 1), &d_act));
    MP_TRY(ws_get(ctx, WS_IO8, 1, &d_out));
    if (n > 0) MP_HIP(hipMemcpyAsync(d_act, actions, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const int tcap = ctx->tree.cap, A = ctx->tree.A, virgin = ctx->tree.virgin;
    if (ctx->tree.il == 2) hipLaunchKernelGGL(uct_path_count_kernel<2>, dim3(1), dim3(1), 0, st, trees, root, tcap, A, d_act, n, d_out, virgin);
    else hipLaunchKernelGGL(uct_path_count_kernel<0>, dim3(1), dim3(1), 0, st, trees, root, tcap, A, d_act, n, d_out, virgin);
    MP_HIP(hipGetLastError());
    MP_HIP(hipMemcpyAsync(count, d_out, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MP_HIP(hipStreamSynchronize(st));
    return MP_OK;
}

int mp_uct_tree_export(mp_ctx *ctx, int32_t root, int32_t cap, int32_t *n_nodes, int32_t *parent, int32_t *action,
                       int64_t *count, double *value, int32_t *first_child, int32_t *n_children)
{
    if (!ctx) return fail(MP_ERR_ARG, "ctx is NULL");
    if (ctx->tree.kind != 1) return fail(MP_ERR_ARG, "mp_uct_tree_export: no UCT tree on this ctx");
    if (root < 0 || root >= ctx->tree.n_roots) return fail(MP_ERR_ARG, "mp_uct_tree_export: root %d out of range", root);
    if (selection_pending(ctx)) return fail(MP_ERR_ARG, "mp_uct_tree_export: a selection of the trees is armed: plan (or mp_uct_reset_tree) first");
    const int tcap = ctx->tree.cap, A = ctx->tree.A;
    std::vector<UctNode> h((size_t)tcap);
    MP_HIP(hipSetDevice(ctx->device));
    MP_HIP(hipStreamSynchronize(ctx->stream));
    const UctNode *trees = (const UctNode *)ctx->ws[ctx->tree.buf ? WS_TREE2 : WS_TREE0].p;
    if (ctx->tree.il == 2) {
        // sibling groups of |A| nodes at stride 64 |A|; group 0 holds the root in its last slot, group g >= 1 the ids 1 + (g-1)|A| ..
        const int groups = (tcap - 1) / A + 1;
        std::vector<UctNode> g((size_t)groups * A);
        MP_HIP(hipMemcpy2D(g.data(), (size_t)A * sizeof(UctNode), trees + ((long)(root >> 6) * (tcap + A) * 64 + (long)(root & 63) * A),
                           (size_t)64 * A * sizeof(UctNode), (size_t)A * sizeof(UctNode), (size_t)groups, hipMemcpyDeviceToHost));
        for (int i = 0; i < tcap; ++i) h[i] = g[(size_t)(i + A - 1)];
    } else
        MP_HIP(hipMemcpy(h.data(), trees + (long)root * tcap, (size_t)tcap * sizeof(UctNode), hipMemcpyDeviceToHost));
    // node slots are appended A at a time; the tree in use is the closure of first_child links.  Slots with
    // count < 0 are the phantoms of actions a listed policy did not list (uct_kernel<.., MK>): they are not nodes.
    // Groups a fresh-tree plan never stored (the children of a count-1 node) get the constant node first.
    const int n = uct_virgin_fill(h.data(), tcap, A, ctx->tree.virgin);
    std::vector<int32_t> id((size_t)n, -1);
    int kept = 0;
    for (int i = 0; i < n; ++i)
        if (h[i].count >= 0) id[i] = kept++;
    if (kept > cap) return fail(MP_ERR_ARG, "mp_uct_tree_export: capacity %d < %d nodes", cap, kept);
    if (parent) parent[0] = -1;
    if (action) action[0] = -1;
    for (int i = 0; i < n; ++i) {
        if (id[i] < 0) continue;
        const int o = id[i];
        if (count) count[o] = h[i].count;
        if (value) value[o] = h[i].value;
        int first = -1, nc = 0;
        if (h[i].first_child >= 0)
            for (int a = 0; a < A; ++a) {
                const int c = id[h[i].first_child + a];
                if (c < 0) continue;
                if (first < 0) first = c;
                ++nc;
                if (parent) parent[c] = o;
                if (action) action[c] = a;
            }
        if (first_child) first_child[o] = first;
        if (n_children) n_children[o] = nc;
    }
    if (n_nodes) *n_nodes = kept;
    return MP_OK;
}

} // extern "C"
