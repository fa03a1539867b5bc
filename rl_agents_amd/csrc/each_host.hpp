// each_host.hpp -- OLOP, BRUE, Sparse Sampling and MDP-GapE on a batch model with one MDP per root (mp_olop_plan_models /
// mp_brue_plan_models / mp_ss_plan_models / mp_gape_plan_models / mp_gape_plan_stochastic_models): the ONE host function that picks
// the kernel form, its grid and its LDS bytes.  The launch code (olop.hip, brue.hip, sparse_sampling.hip, gape.hip, gape_stoch.hip)
// and mp_each_form_info / mp_gape_each_form_info / mp_gape_stoch_each_form_info (no device) call the same function, as opd_shape /
// mp_uct_choose_form do for their planners.
//
// A root of such a call only ever reads ITS MDP's S_each * |A| records.  The "lds" form copies them into the workgroup's LDS
// behind the arrays the kernel already keeps there and serves every model read of the root from LDS; the "global" form is the
// kernel of mp_olop_plan / mp_brue_plan / mp_ss_plan / mp_gape_plan / mp_gape_plan_stochastic on the batch model's global states.
//   MP_EACH_MODEL=lds|global   forces a form where it fits ("lds" is ignored for a table that does not fit LDS)
#pragma once
#include <stdlib.h>
#include <string.h>

#include "common.hpp"

namespace mp {

enum { EACH_OLOP = 0, EACH_BRUE = 1, EACH_SS = 2,
       EACH_GAPE = 3,        // (internal: mp_each_form_info serves the first three; MDP-GapE's query is mp_gape_each_form_info,
       EACH_GAPE_STOCH = 4 }; // that of MDP-GapE with transition bounds mp_gape_stoch_each_form_info)

// Where the LDS form is the DEFAULT: only where it was measured to beat the global form by more than the spread between
// repeated medians (tools/micro_each.py -> profiles/each_model_ab.json; the highway shape, 120 states x
// 5 actions = 9.6 KB a table, 1 to 65 536 roots):
//   * a workgroup of at most kLdsBytes / 16 bytes, the footprint measured: 16 wavefronts stay resident on a CU.  A larger table
//     leaves fewer, and its copy costs more than the few hundred records a plan reads of it: not measured, not the default;
//   * OLOP at every batch size (0.3 - 6.6 % faster); BRUE (0.7 - 3.3 %) only while every root's workgroup is resident at once --
//     at 65 536 roots, where the LDS form halves the resident wavefronts, the difference was inside the spread;
//   * Sparse Sampling (tools/micro_ss_each.py -> profiles/ss_each_ab.json; horizon 3, C 3) as BRUE: 2.2 % faster at 1
//     and 256 roots and 4.4 % at 4 096 = 256 CUs x 16, each beyond the spread (0.2 % / 3.3 % of the time); at 65 536 roots, where
//     a workgroup of 9 792 bytes leaves 16 wavefronts resident on a CU against the global form's 32, it was 0.3 % SLOWER.
//     (Smaller tables take the LDS form by the same rule; only this footprint was measured.)
//   * MDP-GapE (tools/micro_gape_each.py -> profiles/gape_each_ab.json; the reference's highway baseline: horizon
//     6, 14 episodes, accuracy 0.1): 1.1 % faster at 256 roots and 3.8 % at 4 096 = 256 CUs x 16, each beyond the spread (0.7 % /
//     1.9 % of the time); at 1 root the 1.0 % it was ahead lay inside the spread (3.3 %), and at 65 536 roots, where a workgroup
//     of 9 632 bytes leaves 17 to a CU against the global form's 32, it was 33 % SLOWER.  So: from kGapeLdsMinRoots roots on,
//     and, as BRUE, only while every root's workgroup is resident at once.
//   * MDP-GapE with transition bounds (mp_gape_plan_stochastic_models; tools/micro_gape_stoch_each.py ->
//     profiles/gape_stoch_each_ab.json; horizon 3, 20 episodes, accuracy 0, max_next_states_count 2) as MDP-GapE:
//     1.1 % faster at 256 roots and 4.1 % at 4 096, each beyond the spread (0.3 % / 1.9 % of the time); at 1 root the 1.4 % it was
//     ahead lay inside the spread (2.0 %), and at 65 536 roots, where a workgroup of 9 632 bytes leaves 17 to a CU against the
//     global form's 32, it was 21 % SLOWER.  So: from kGapeLdsMinRoots roots on, only while every root's workgroup is resident.
// MP_EACH_MODEL=lds takes the LDS form for any table that fits the CU's LDS.
constexpr size_t kEachLdsDefaultBytes = kLdsBytes / 16;
constexpr int kGapeLdsMinRoots = 256; // MDP-GapE, with or without transition bounds: the smallest batch at which the LDS form was
                                      // measured ahead beyond the spread

struct EachForm {
    size_t arrays;   // bytes of the kernel's own LDS arrays (OLOP, MDP-GapE: path[L + 1] int32, with transition bounds path[2 * H + 1];
                     // BRUE: rew[H] f64 + po[H] int2, Sparse Sampling: H frames of 64 bytes), 16-byte rounded
    size_t lds_need; // arrays + S_each * |A| * 16: what a workgroup of the LDS form takes
    bool lds;        // the form of this call
    int grid;        // workgroups launched (one wavefront each): what is resident, at most n_roots
    size_t lds_bytes() const { return lds ? lds_need : arrays; } // dynamic LDS of the launch
};

inline size_t each_kernel_arrays(int planner, int horizon)
{
    const size_t raw = planner == EACH_OLOP || planner == EACH_GAPE ? (size_t)(horizon + 1) * sizeof(int32_t)
                     : planner == EACH_GAPE_STOCH ? (size_t)(2 * horizon + 1) * sizeof(int32_t)
                     : planner == EACH_BRUE ? (size_t)horizon * (sizeof(double) + 2 * sizeof(int32_t)) : (size_t)horizon * 64;
    return (raw + 15) & ~(size_t)15;
}

inline EachForm each_form(int planner, int S_each, int A, int horizon, int n_roots, int cus)
{
    EachForm f;
    f.arrays = each_kernel_arrays(planner, horizon);
    f.lds_need = f.arrays + (size_t)S_each * A * sizeof(Rec);
    const bool fits = f.lds_need <= kLdsBytes;
    const long lds_per_cu = fits ? (long)(kLdsBytes / f.lds_need < 32 ? kLdsBytes / f.lds_need : 32) : 0;
    // (BRUE, Sparse Sampling, MDP-GapE: only while every root's workgroup is resident at once; MDP-GapE, with or without
    // transition bounds: from 256 roots on)
    f.lds = fits && f.lds_need <= kEachLdsDefaultBytes && (planner == EACH_OLOP || (long)n_roots <= (long)cus * lds_per_cu) &&
            ((planner != EACH_GAPE && planner != EACH_GAPE_STOCH) || n_roots >= kGapeLdsMinRoots);
    if (const char *force = getenv("MP_EACH_MODEL")) {
        if (!strcmp(force, "lds")) f.lds = fits;
        else if (!strcmp(force, "global")) f.lds = false;
    }
    const long resident = (long)cus * (f.lds ? lds_per_cu : 32);
    f.grid = (int)(n_roots < resident ? n_roots : resident);
    return f;
}

// the global form whatever the table and the knob: the launch of mp_olop_plan / mp_brue_plan / mp_ss_plan / mp_gape_plan /
// mp_gape_plan_stochastic themselves
inline EachForm each_form_global(int planner, int horizon, int n_roots, int cus)
{
    EachForm f;
    f.arrays = f.lds_need = each_kernel_arrays(planner, horizon);
    f.lds = false;
    const long resident = (long)cus * 32;
    f.grid = (int)(n_roots < resident ? n_roots : resident);
    return f;
}

} // namespace mp
