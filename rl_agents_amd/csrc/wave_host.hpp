// wave_host.hpp -- the host side that the wave-per-root planners share (mp_olop_plan, mp_brue_plan, mp_ss_plan, mp_gbopd_plan:
// one root or planner per 64-lane workgroup): the memory flags and root states of a call, the view of a finite MDP, the staging
// of roots, generator records and results, the tree workspace, the launch, and the head of a tree export.  Each entry point
// keeps its NULL check, its own size checks and messages between the shared ones, its tables, its args struct and its kernels.
#pragma once
#include "common.hpp"

namespace mp {

// ---- call prologue, in two parts: an entry point checks its model and sizes between them.  `who` is its name in the messages.
inline int wave_mem(const char *who, int32_t *mem, int *rmem)
{
    if (!mem_valid(*mem)) return fail(MP_ERR_ARG, "%s: unknown mem flags %d", who, *mem);
    *rmem = mem_rng(*mem); *mem = mem_arrays(*mem);
    return MP_OK;
}

// root states in a host array are range-checked against S here, unless the array lives in mp_host_alloc memory (the kernel
// reads that one in place, as it reads a device array); then the device is made current: what follows in the caller may use it
inline int wave_roots(mp_ctx *ctx, const char *who, const int32_t *root_state, int n_roots, int S, int mem)
{
    if (mem == MP_MEM_HOST && !pinned_alias(ctx, root_state, (size_t)n_roots * sizeof(int32_t)))
        for (int i = 0; i < n_roots; ++i)
            if (root_state[i] < 0 || root_state[i] >= S) return fail(MP_ERR_ARG, "%s: root state %d out of range", who, root_state[i]);
    MP_HIP(hipSetDevice(ctx->device));
    return MP_OK;
}

// ---- a finite MDP as BRUE and Sparse Sampling read it: tables, dense or sparse rows.  wave_mdp_check refuses what is not one
// whole model (`each`: a batch model of one MDP per root is one, too); wave_mdp, once the device is current, builds the sampling
// thresholds a dense / sparse model needs and fills the six fields BrueArgs and SsArgs share (W: the length of a threshold row).
inline int wave_mdp_check(const char *who, const mp_model *model, bool each)
{
    if (model->mode != MP_MODE_DETERMINISTIC && model->mode != MP_MODE_STOCHASTIC && model->mode != MP_MODE_SPARSE)
        return fail(MP_ERR_MODE, "%s: model mode %d is not a finite MDP", who, model->mode);
    if (model->M != 1 || (!each && model->NB != 1) || (model->mode == MP_MODE_STOCHASTIC && model->Sc != model->S))
        return fail(MP_ERR_MODE, "%s: one whole model expected (no joint, batch or row-block model)", who);
    return MP_OK;
}

template <typename Args>
inline int wave_mdp(mp_ctx *ctx, const char *who, mp_model *model, Args *a)
{
    if (model->mode != MP_MODE_DETERMINISTIC) MP_TRY(ensure_thresholds(ctx, who, model));
    a->mode = model->mode; a->W = model->mode == MP_MODE_STOCHASTIC ? model->S : model->B;
    a->rec = model->rec; a->thr = model->thr; a->nxt = model->NXT; a->R = model->R;
    return MP_OK;
}

// ---- the caller's arrays of a plan call and their device side, named once: inputs (root states, optional ones such as
// root_steps), the generator records (in and out, following their own flag rmem: MP_MEM_RNG_DEVICE is an mp_rng) and the results
// a planner adds, `per_root` elements a root, each with the workspace slot that backs a host array.  The generator records are
// named before the results.  (mp_uct_plan reads the same table with a staging of its own: uct.hip.)
struct WaveIo {
    enum { IN = 1, OUT = 2 };
    struct Item {
        void *host; void **dev;   // the caller's array (NULL: an optional one left out) and where the args struct keeps its device side
        size_t per_root;          // bytes a root
        int slot, dir, mem;       // workspace slot; IN, OUT or both; the memory flag it follows
        char *base;               // mp_uct_plan: the device side of root 0 (*dev moves from chunk to chunk)
    };
    Item item[12];
    int n = 0, mem, rmem, n_roots;
    size_t bytes(const Item &t) const { return n_roots * t.per_root; }
    template <typename T, typename D>
    void put(int slot, T *host, D **dev, size_t per_root, int dir, int flag)
    {
        item[n++] = {(void *)host, (void **)dev, per_root * sizeof(T), slot, dir, flag, nullptr};
    }
    template <typename T, typename D>
    void add(int slot, T *host, D **dev, size_t per_root = 1) { put(slot, host, dev, per_root, OUT, mem); }   // a result
    template <typename T, typename D>
    void in(int slot, T *host, D **dev, size_t per_root = 1) { put(slot, host, dev, per_root, IN, mem); }     // an input
    template <typename D>
    void rng(uint64_t *rng_state, D **d_rng) { put(WS_IO2, rng_state, d_rng, 6, IN | OUT, rmem); }
    WaveIo(int mem, int rmem, int n_roots) : mem(mem), rmem(rmem), n_roots(n_roots) {}
    WaveIo(int mem, int rmem, int n_roots, const int32_t *root_state, const int32_t **d_root_state, uint64_t *rng_state, uint64_t **d_rng)
        : WaveIo(mem, rmem, n_roots)
    {
        in(WS_IO0, root_state, d_root_state);
        rng(rng_state, d_rng);
    }
};

inline int wave_stage(mp_ctx *ctx, const WaveIo &io)
{
    for (int i = 0; i < io.n; ++i) {
        const WaveIo::Item &t = io.item[i];
        char *d = nullptr; // (an array left out stays null: the kernels skip it)
        if (t.host && (t.dir & WaveIo::IN)) MP_TRY(stage_in(ctx, t.slot, (const char *)t.host, io.bytes(t), t.mem, &d));
        else if (t.host) MP_TRY(stage_out_alloc(ctx, t.slot, (char *)t.host, io.bytes(t), t.mem, &d));
        *t.dev = d; // (stored as a void *: the type that may alias the args struct's pointer of any type)
    }
    return MP_OK;
}

// the generator records back first, then the results in the order they were named; host arrays are complete on return
inline int wave_unstage(mp_ctx *ctx, const WaveIo &io)
{
    for (int i = 0; i < io.n; ++i) {
        const WaveIo::Item &t = io.item[i];
        if (t.dir & WaveIo::OUT) MP_TRY(stage_out_copy(ctx, (char *)t.host, (const char *)*t.dev, io.bytes(t), t.mem));
    }
    if (io.mem == MP_MEM_HOST) MP_HIP(hipStreamSynchronize(ctx->stream));
    return MP_OK;
}

// ---- tree workspace of OLOP, BRUE and Sparse Sampling: nodes [slots][cap] in WS_TREE0, a second array of `aux_per_node` X per
// node in WS_TREE1 (none when `aux` is null) and the node counts [n_roots] in WS_TREE7.  Every root has a slot of its own while
// the batch's trees fit `keep_limit` bytes (-> true, ctx->tree.K = -1); else there are `slots_else` of them and root 0's is
// `slot0` (ctx->tree.K), the tree an export can still read.
template <typename N, typename X>
inline int wave_tree(mp_ctx *ctx, int kind, int n_roots, int A, long cap, size_t aux_per_node, size_t keep_limit, int slots_else,
                     int slot0, N **nodes, X **aux, int32_t **n_nodes_out, int *keep)
{
    *keep = (size_t)n_roots * ((size_t)cap * (sizeof(N) + aux_per_node * sizeof(X))) <= keep_limit;
    const size_t slots = *keep ? (size_t)n_roots : (size_t)slots_else;
    MP_TRY(ws_get(ctx, WS_TREE0, slots * cap, nodes));
    if (aux) MP_TRY(ws_get(ctx, WS_TREE1, slots * cap * aux_per_node, aux));
    MP_TRY(ws_get(ctx, WS_TREE7, (size_t)n_roots, n_nodes_out));
    ctx->tree.kind = kind; ctx->tree.armed = false; ctx->tree.n_src = 0; ctx->tree.n_roots = n_roots; ctx->tree.A = A; ctx->tree.cap = (int)cap;
    ctx->tree.K = *keep ? -1 : slot0;
    return MP_OK;
}

// ---- launch tail: `grid` workgroups of one wavefront with `lds` bytes of dynamic LDS, recorded as `form`
template <typename Args>
inline int wave_launch(mp_ctx *ctx, void (*kfn)(Args), int grid, size_t lds, const FormName &form, const Args &a)
{
    if (lds > 64 * 1024)
        MP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    form_record(ctx->last_variant, form);
    MP_TRY(kernels_begin(ctx));
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(64), lds, ctx->stream, a);
    MP_TRY(kernels_end(ctx, 1));
    MP_HIP(hipGetLastError());
    return MP_OK;
}

// ---- tree export: every check up to the node count of `root`, whose tree sits in *slot of the arrays wave_tree reserved
// (`who` is the export's name, `plan` the entry point whose tree it reads).  The capacity check and *n_nodes stay with the export.
inline int wave_export_begin(mp_ctx *ctx, int kind, const char *who, const char *plan, int root, int32_t *slot, int32_t *n)
{
    if (!ctx) return fail(MP_ERR_ARG, "ctx is NULL");
    if (ctx->tree.kind != kind) return fail(MP_ERR_ARG, "%s: no tree of %s on this ctx", who, plan);
    if (root < 0 || root >= ctx->tree.n_roots) return fail(MP_ERR_ARG, "%s: root %d out of range", who, root);
    if (ctx->tree.K >= 0 && root != 0)
        return fail(MP_ERR_ARG, "%s: the batch's trees did not all fit the workspace; only root 0's was kept", who);
    *slot = ctx->tree.K < 0 ? root : ctx->tree.K;
    MP_HIP(hipSetDevice(ctx->device));
    MP_HIP(hipStreamSynchronize(ctx->stream));
    MP_HIP(hipMemcpy(n, (const int32_t *)ctx->ws[WS_TREE7].p + root, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*n < 1 || *n > ctx->tree.cap) return fail(MP_ERR_ARG, "%s: bad node count %d", who, *n);
    return MP_OK;
}

// the first n elements of `elt` bytes of slot `slot` of a per-slot array (WS_TREE0 / WS_TREE1)
inline int wave_pull(mp_ctx *ctx, int ws_slot, int slot, int n, size_t elt, void *dst)
{
    MP_HIP(hipMemcpy(dst, (const char *)ctx->ws[ws_slot].p + (size_t)slot * ctx->tree.cap * elt, (size_t)n * elt, hipMemcpyDeviceToHost));
    return MP_OK;
}

} // namespace mp
