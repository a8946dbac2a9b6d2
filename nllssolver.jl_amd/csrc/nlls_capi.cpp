// nlls_capi.cpp -- the extern "C" boundary declared in include/nlls_amd.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>

#include "nlls_internal.hpp"

using namespace nlls;

namespace {
constexpr int32_t NLLS_MAX_GRAPH_NODES = 1 << 27;      // nlls_rcm_order / nlls_nd_tiles: nodes of a reduced-system graph
int fail(nlls_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; return code; }
// (every entry point launches on ctx->stream: make the context's device current first -- two contexts on different devices in one
// process, or a caller that changed the current device, must not end up on a foreign stream)
#define NEED_READY() do { if (!ctx) return NLLS_ERR_INVALID_ARG; if (!ctx->ready) return fail(ctx, NLLS_ERR_NOT_READY, "nlls_upload_structure has not succeeded"); (void)hipSetDevice(ctx->device); } while (0)
#define NEED_GRAD_LAZY() do { NEED_READY(); if (!ctx->lin.have) return fail(ctx, NLLS_ERR_NOT_READY, "nlls_sweep_gradhess has not been run"); } while (0)
// (... and with the reduced rows summed over ranks: every entry point but the LM trial itself reads them as if one GPU had swept all cost blocks)
#define NEED_GRAD() do { NEED_GRAD_LAZY(); TRY(ensure_grad(ctx, 2)); TRY(ensure_reduced_summed(ctx)); } while (0)
#define TRY(expr) do { int rc_ = (expr); if (rc_ != NLLS_OK) return rc_; } while (0)

// copy `count` scalars starting at `slot` to the pinned mirror and wait
int fetch_scalars(nlls_ctx* ctx, int slot, int count) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars + slot, ctx->scalars.p + slot, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
}
bool valid_set(int w) { return w >= 0 && w < 3; }
// Whoever needs A and b for the CURRENT point comes through here.  `level` (nlls::Linearisation): 1 -- the reduced rows suffice (the matrix-free LM trial); 2 -- all of
// A.data and b.  Less than is asked for is swept (again) here, at CURRENT: the matrix-free trial never forms the eliminated rows, and nlls_sweep_gradhess(ctx, NULL) defers it.
int ensure_grad(nlls_ctx* ctx, int level) {
    lookahead_consume(ctx, true);
    if (ctx->lin.level >= level && ctx->lin.phys == ctx->vars_slot[NLLS_VARS_CURRENT]) return NLLS_OK;
    return enqueue_sweep_gradhess(ctx, false, NLLS_VARS_CURRENT, level == 1 ? 1 : 0);
}
// phase events (nlls_ctx::phase_on): record event k on the stream
void phase_mark(nlls_ctx* ctx, int k) { if (ctx->phase_on && (size_t)k < ctx->phase_ev.size()) (void)hipEventRecord(ctx->phase_ev[k], ctx->stream); }
// is this trial matrix-free?  (nlls_ctx::mf_ok: the structure qualifies; mf_on: not switched off; the trial starts at CURRENT, one rank, no collective route)
// nlls_eval_jacobians / nlls_eval_gradhess: everything checked on the host before anything is enqueued or written; then the listed blocks to the device, one launch
// (nlls_linearize.hip), the records home.  out[k] (null: not wanted) takes rec[k] doubles per block.  Reads only: no event of nlls_state.hpp.
int linearize_call(nlls_ctx* ctx, const char* name, int32_t which, int32_t group, int64_t n, const int64_t* index, bool jac, double* const out[3]) {
    const std::string nm(name);
    if (!valid_set(which)) return fail(ctx, NLLS_ERR_INVALID_ARG, nm + ": bad variable set");
    if (!out[0] && !out[1] && !out[2]) return fail(ctx, NLLS_ERR_INVALID_ARG, nm + ": no output asked for");
    if (ctx->nranks > 1) return fail(ctx, NLLS_ERR_UNSUPPORTED, nm + " under nlls_set_shard: a rank holds only its own cost blocks");
    if (group < 0 || group >= (int32_t)ctx->groups.size()) return fail(ctx, NLLS_ERR_INVALID_ARG, nm + ": bad cost group");
    const Group& G = ctx->groups[(size_t)group];
    LinSizes s;
    if (is_dyn_kind(G.res_kind) || !lin_sizes(G.res_kind, s)) return fail(ctx, NLLS_ERR_UNSUPPORTED, nm + ": the Jacobian of a dynamic-size kind is its own payload");
    if (jac && s.m == 0) return fail(ctx, NLLS_ERR_UNSUPPORTED, nm + ": a non-squared cost kind has no residual");
    if (n < 0 || (!index && n > G.ncost)) return fail(ctx, NLLS_ERR_INVALID_ARG, nm + ": n outside 0 .. ncost");
    if (n == 0) return NLLS_OK;
    std::vector<int64_t> blocks;                        // the listed blocks as they were checked (any order, repeats allowed: nothing is written through them)
    if (index) { blocks.assign(index, index + n);
        for (int64_t k : blocks) if (k < 1 || k > G.ncost) return fail(ctx, NLLS_ERR_INVALID_ARG, nm + ": index outside 1 .. ncost"); }
    const size_t rec[3] = {jac ? (size_t)s.m : 1, jac ? (size_t)s.m * (size_t)s.nj : (size_t)s.p, jac ? 0 : (size_t)s.p * (size_t)s.p};
    size_t need = 0, off[3]; double bytes = 0;
    for (int k = 0; k < 3; ++k) { off[k] = need; if (out[k]) { need += (size_t)n * rec[k]; bytes += 8.0 * (double)n * (double)rec[k]; } }
    // (DevBuf::alloc records the new size before it allocates: a buffer that could not be had is released, so that the next call asks again instead of launching on null)
    if (ctx->lin_out.n < need || !ctx->lin_out.p) { const hipError_t e = ctx->lin_out.alloc(need); if (e != hipSuccess) { ctx->lin_out.release(); (void)hipGetLastError(); return hip_fail(ctx, e, (nm + ": scratch for the records").c_str()); } }
    if (index && (ctx->lin_index.n < (size_t)n || !ctx->lin_index.p)) { const hipError_t e = ctx->lin_index.alloc((size_t)n); if (e != hipSuccess) { ctx->lin_index.release(); (void)hipGetLastError(); return hip_fail(ctx, e, (nm + ": scratch for the index").c_str()); } }
    if (index) HIP_TRY(ctx, hipMemcpyAsync(ctx->lin_index.p, blocks.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    double* d[3]; for (int k = 0; k < 3; ++k) d[k] = out[k] ? ctx->lin_out.p + off[k] : nullptr;
    if (jac) TRY(enqueue_linearize(ctx, G, which, n, index ? ctx->lin_index.p : nullptr, d[0], d[1], nullptr, nullptr, nullptr));
    else TRY(enqueue_linearize(ctx, G, which, n, index ? ctx->lin_index.p : nullptr, nullptr, nullptr, d[0], d[1], d[2]));
    if (ctx->phase_on) ctx->lin_bytes = bytes;          // (beside the event pair: nlls_get_phase_times [10], [11])
    if (jac) { if (out[1]) ctx->lin_batch[0] = s.batch_j; } else { if (out[1]) ctx->lin_batch[1] = s.batch_g; if (out[2]) ctx->lin_batch[2] = s.batch_h; }
    for (int k = 0; k < 3; ++k) if (out[k]) HIP_TRY(ctx, hipMemcpyAsync(out[k], d[k], sizeof(double) * (size_t)n * rec[k], hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (`blocks` and the caller's arrays are in use until here)
    return NLLS_OK;
}
// staging of the matrix-free products' vectors: grown on demand, kept until the next upload (a buffer that could not be had is released, as in linearize_call)
int apply_io(nlls_ctx* ctx, size_t need, double** out) {
    DevBuf<double>& io = ctx->app.io;
    if (io.n < need || !io.p) { const hipError_t e = io.alloc(need); if (e != hipSuccess) { io.release(); (void)hipGetLastError(); return hip_fail(ctx, e, "matrix-free products: staging for the vectors"); } }
    *out = io.p; return NLLS_OK;
}
bool mf_trial(const nlls_ctx* ctx, int32_t from) { return ctx->mf_ok && ctx->sw.mf_on && !ctx->lin.stale_point && from == NLLS_VARS_CURRENT && ctx->nranks == 1 && !ctx->reduce_fn && ctx->info.is_sparse && !ctx->tiny_dense; }
}  // namespace

extern "C" {

int nlls_ctx_create(const int32_t* device_ids, int32_t ndev, nlls_ctx** out) { NLLS_API_BEGIN
    if (!out) return NLLS_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return NLLS_ERR_NO_DEVICE;   // never falls back to a CPU path
    int dev = (device_ids && ndev > 0) ? device_ids[0] : 0;
    if (dev < 0 || dev >= count) return NLLS_ERR_INVALID_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return NLLS_ERR_HIP;
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return NLLS_ERR_NO_DEVICE;  // the code object is gfx950-only
    nlls_ctx* c = new (std::nothrow) nlls_ctx();
    if (!c) return NLLS_ERR_HIP;
    c->device = dev; c->num_cus = prop.multiProcessorCount;
    { int khz = 100000; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000; c->tb_ns_per_tick = 1e6 / (double)khz; }
    read_create_env(c->sw);
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return NLLS_ERR_HIP; }
    c->own_stream = true;
    if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) { delete c; return NLLS_ERR_HIP; }
    *out = c;
    return NLLS_OK;
    NLLS_API_END(nullptr)
}

int nlls_ctx_destroy(nlls_ctx* ctx) { NLLS_API_BEGIN
    if (!ctx) return NLLS_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    comm_release(ctx);
    if (ctx->h_scalars) (void)hipHostFree(ctx->h_scalars);
    if (ctx->stream2) { (void)hipStreamSynchronize(ctx->stream2); (void)hipStreamDestroy(ctx->stream2); }
    for (auto& e : ctx->prof_ev) (void)hipEventDestroy(e);
    for (auto& e : ctx->phase_ev) (void)hipEventDestroy(e);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    hipStream_t s = ctx->own_stream ? ctx->stream : nullptr;
    delete ctx;
    if (s) (void)hipStreamDestroy(s);
    return NLLS_OK;
    NLLS_API_END(ctx)
}

const char* nlls_last_error(const nlls_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int nlls_set_stream(nlls_ctx* ctx, void* hip_stream) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->own_stream && ctx->stream) { (void)hipStreamDestroy(ctx->stream); ctx->own_stream = false; }
    if (hip_stream) ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    else { if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return NLLS_ERR_HIP; ctx->own_stream = true; }
    return NLLS_OK;
    NLLS_API_END(ctx)
}

int nlls_set_shard(nlls_ctx* ctx, int32_t rank, int32_t nranks) { NLLS_API_BEGIN
    if (!ctx || nranks < 1 || rank < 0 || rank >= nranks) return NLLS_ERR_INVALID_ARG;
    ctx->rank = ctx->shard_rank = rank; ctx->nranks = ctx->shard_nranks = nranks; ctx->replicated = false; ctx->ready = false;
    return NLLS_OK;
    NLLS_API_END(ctx)
}

int nlls_var_storage(int32_t k, int32_t d) { NLLS_API_BEGIN return var_storage(k, d); NLLS_API_END(nullptr) }
int nlls_var_dof(int32_t k, int32_t d) { NLLS_API_BEGIN return var_dof(k, d); NLLS_API_END(nullptr) }
int nlls_robust_nparams(int32_t k) { NLLS_API_BEGIN return robust_nparams(k) >= 0 ? robust_nparams(k) : NLLS_ERR_UNSUPPORTED; NLLS_API_END(nullptr) }
int nlls_res_ndeps(int32_t k) { NLLS_API_BEGIN ResDesc d; return res_desc(k, d) ? d.ndeps : NLLS_ERR_UNSUPPORTED; NLLS_API_END(nullptr) }
int nlls_res_nres(int32_t k) { NLLS_API_BEGIN ResDesc d; return res_desc(k, d) ? d.nres : NLLS_ERR_UNSUPPORTED; NLLS_API_END(nullptr) }
int nlls_res_ndata(int32_t k) { NLLS_API_BEGIN ResDesc d; return res_desc(k, d) ? d.ndata : NLLS_ERR_UNSUPPORTED; NLLS_API_END(nullptr) }
int nlls_res_jac_cols(int32_t k) { NLLS_API_BEGIN LinSizes z; return lin_sizes(k, z) ? z.nj : NLLS_ERR_UNSUPPORTED; NLLS_API_END(nullptr) }
int nlls_res_gh_dim(int32_t k) { NLLS_API_BEGIN LinSizes z; return lin_sizes(k, z) ? z.p : NLLS_ERR_UNSUPPORTED; NLLS_API_END(nullptr) }
int nlls_res_slot_kind(int32_t k, int32_t slot, int32_t* vk, int32_t* vd) { NLLS_API_BEGIN
    ResDesc d; if (!res_desc(k, d)) return NLLS_ERR_UNSUPPORTED;
    if (slot < 0 || slot >= d.ndeps) return NLLS_ERR_INVALID_ARG;
    if (vk) *vk = d.sk[slot]; if (vd) *vd = d.sd[slot];
    return NLLS_OK;
    NLLS_API_END(nullptr)
}
int nlls_rcm_order(int32_t n, const int64_t* adjptr, const int32_t* adj, int32_t* perm_out) { NLLS_API_BEGIN
    if (n < 0 || (n > 0 && (!adjptr || !perm_out))) return NLLS_ERR_INVALID_ARG;
    if (n > NLLS_MAX_GRAPH_NODES) return NLLS_ERR_INVALID_ARG;          // (a size no reduced system has: refused before any work vector is sized by it)
    std::vector<std::vector<int32_t>> a((size_t)n);
    for (int32_t i = 0; i < n; ++i) { if (adjptr[i + 1] < adjptr[i]) return NLLS_ERR_INVALID_ARG;
        for (int64_t q = adjptr[i]; q < adjptr[i + 1]; ++q) { if (adj[q] < 0 || adj[q] >= n || adj[q] == i) return NLLS_ERR_INVALID_ARG; a[i].push_back(adj[q]); } }
    const std::vector<int32_t> p = nlls::rcm_order(a);
    for (int32_t i = 0; i < n; ++i) perm_out[i] = p[i];
    return NLLS_OK;
    NLLS_API_END(nullptr)
}

int nlls_nd_tiles(int32_t n, int32_t nborder, const int64_t* adjptr, const int32_t* adj, const int32_t* dof, int32_t* tile_of, int32_t* row_in_tile,
                  int32_t max_tiles, int32_t* parent, int32_t* level, int64_t* colptr, int64_t max_rows, int32_t* rows) {
    if (n > NLLS_MAX_GRAPH_NODES || nborder > NLLS_MAX_GRAPH_NODES) return NLLS_ERR_INVALID_ARG;
    if (n < 0 || nborder < 0 || (n > 0 && !adjptr) || (n + nborder > 0 && (!dof || !tile_of || !row_in_tile)) || !parent || !level || !colptr || (max_rows > 0 && !rows)) return NLLS_ERR_INVALID_ARG;
    std::vector<std::vector<int32_t>> a((size_t)n);
    for (int32_t i = 0; i < n; ++i) { if (adjptr[i + 1] < adjptr[i]) return NLLS_ERR_INVALID_ARG;
        for (int64_t q = adjptr[i]; q < adjptr[i + 1]; ++q) { if (adj[q] < 0 || adj[q] >= n || adj[q] == i) return NLLS_ERR_INVALID_ARG; a[i].push_back(adj[q]); }
        std::sort(a[i].begin(), a[i].end()); a[i].erase(std::unique(a[i].begin(), a[i].end()), a[i].end()); }
    nlls::TspSym sym; nlls::Switches sw; read_upload_env(sw);
    if (!nlls::tsp_symbolic(a, std::vector<int32_t>(dof, dof + n + nborder), nborder, sym, sw)) return NLLS_ERR_INVALID_ARG;
    if (sym.nt > max_tiles || sym.ntiles_lower - sym.nt > max_rows) return NLLS_ERR_INVALID_ARG;
    for (int32_t i = 0; i < n + nborder; ++i) { tile_of[i] = sym.tile_of[i]; row_in_tile[i] = sym.row_in_tile[i]; }
    colptr[0] = 0;
    for (int k = 0; k < sym.nt; ++k) { parent[k] = sym.parent[k]; level[k] = sym.level[k]; int64_t q = colptr[k]; for (int32_t t : sym.cstruct[k]) rows[q++] = t; colptr[k + 1] = q; }
    return sym.nt;
}

int nlls_upload_structure(nlls_ctx* ctx, int64_t nvar, const int32_t* var_kind, const int32_t* var_dim, const uint64_t* blockindices,
                          int32_t ngroups, const nlls_cost_group* groups, int32_t flags) {
    if (!ctx || nvar < 0 || ngroups < 0 || (nvar && (!var_kind || !var_dim || !blockindices)) || (ngroups && !groups)) return NLLS_ERR_INVALID_ARG;
    try {
        (void)hipSetDevice(ctx->device);
        read_upload_env(ctx->sw);                // (the upload-time switches hold for this upload; what nlls_ctx_create read and nlls_set_option wrote stays)
        ctx->err_sub = NLLS_SUB_NONE;
        int rc = build_structure(ctx, nvar, var_kind, var_dim, blockindices, ngroups, groups, flags);
        // an eliminated block with more neighbours than the Schur kernels stage in LDS: solve the full system instead of failing
        // (decided on the sub-code the structure builder left, not on the error text; the retry declines by itself -- dense size
        // guard in build_schur -- when the full system is too large to factor densely)
        if (rc == NLLS_ERR_UNSUPPORTED && !(flags & NLLS_FLAG_NO_SCHUR) && ctx->err_sub == NLLS_SUB_SCHUR_SHAPE) {
            ctx->err_sub = NLLS_SUB_NONE;
            rc = build_structure(ctx, nvar, var_kind, var_dim, blockindices, ngroups, groups, flags | NLLS_FLAG_NO_SCHUR);
        }
        return rc;
    }
    catch (const std::exception& e) { return fail(ctx, NLLS_ERR_HIP, std::string("host exception: ") + e.what()); }
    catch (...) { return nlls::api_exception(ctx, "unknown C++ exception"); }
}

int nlls_get_info(const nlls_ctx* ctx, nlls_info* out) { NLLS_API_BEGIN
    if (!ctx || !out || !ctx->ready) return ctx ? NLLS_ERR_NOT_READY : NLLS_ERR_INVALID_ARG;
    *out = ctx->info; return NLLS_OK;
    NLLS_API_END(const_cast<nlls_ctx*>(ctx))
}

int nlls_get_bsm_index(const nlls_ctx* ctx, int64_t* colptr, int64_t* rowval, int64_t* nzval, int64_t* boffsets) { NLLS_API_BEGIN
    if (!ctx || !ctx->ready) return ctx ? NLLS_ERR_NOT_READY : NLLS_ERR_INVALID_ARG;
    if (ctx->info.is_sparse) {
        if (colptr) for (size_t i = 0; i < ctx->it_colptr.size(); ++i) colptr[i] = ctx->it_colptr[i] + 1;
        if (rowval) for (size_t i = 0; i < ctx->it_rowval.size(); ++i) rowval[i] = ctx->it_rowval[i] + 1;
        if (nzval) for (size_t i = 0; i < ctx->it_nzval.size(); ++i) nzval[i] = ctx->it_nzval[i] + 1;
    }
    if (boffsets) for (int64_t i = 0; i < ctx->info.nblocks; ++i) boffsets[i] = ctx->boffsets[i] + 1;
    return NLLS_OK;
    NLLS_API_END(const_cast<nlls_ctx*>(ctx))
}

int nlls_set_variables(nlls_ctx* ctx, int32_t which, const double* packed) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(which) || !packed) return NLLS_ERR_INVALID_ARG;
    TRY(vars_written(ctx, which));
    if (which == NLLS_VARS_CURRENT) { new_starting_point(ctx); ctx->tb_prev_end = 0.0; }
    HIP_TRY(ctx, hipMemcpyAsync(vars_ptr(ctx, which), packed, sizeof(double) * ctx->info.var_storage, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_get_variables(nlls_ctx* ctx, int32_t which, double* packed) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(which) || !packed) return NLLS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(packed, vars_ptr(ctx, which), sizeof(double) * ctx->info.var_storage, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_swap_variables(nlls_ctx* ctx, int32_t a, int32_t b) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(a) || !valid_set(b)) return NLLS_ERR_INVALID_ARG;
    std::swap(ctx->vars_slot[a], ctx->vars_slot[b]); return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_copy_variables(nlls_ctx* ctx, int32_t dst, int32_t src) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(dst) || !valid_set(src)) return NLLS_ERR_INVALID_ARG;
    if (dst != src) TRY(vars_written(ctx, dst));
    if (dst != src) HIP_TRY(ctx, hipMemcpyAsync(vars_ptr(ctx, dst), vars_ptr(ctx, src), sizeof(double) * ctx->info.var_storage, hipMemcpyDeviceToDevice, ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}

// Lazy stage 0 (collective route): nlls_sweep_gradhess(ctx, NULL) leaves the reduced rows of A.data and b as this rank's share -- all an LM trial
// takes from them is linear in them (the reduced-reduced blocks and b_R enter [S | s], which is summed over ranks anyway; x'Hx and g'x are sums of
// the ranks' scalars), so the per-iteration all-reduce of [cost | reduced rows | reduced b] and its pack / unpack launches are skipped.  Whatever else
// reads them (the initial damping's max |diag|, nlls_get_grad, nlls_solve, ...) sums them first, here: a collective -- every rank makes the same calls.
static int ensure_reduced_summed(nlls_ctx* ctx) {
    if (ctx->lin.summed) return NLLS_OK;
    new_linearisation(ctx, true, false);     // (the same linearisation, its reduced rows summed from here on)
    if (!ctx->reduce_fn || ctx->nranks <= 1) return NLLS_OK;
    ctx->n_stage0++;
    TRY(enqueue_pack_reduce0(ctx)); TRY(comm_reduce(ctx, ctx->redbuf.p, ctx->redbuf_len, NLLS_REDUCE_SUM)); TRY(enqueue_unpack_reduce0(ctx, false));
    return NLLS_OK;
}
int nlls_sweep_gradhess(nlls_ctx* ctx, double* cost_out) { NLLS_API_BEGIN
    NEED_READY();
    if (sweep_asked(ctx, cost_out != nullptr)) { new_linearisation(ctx); return NLLS_OK; }   // (already enqueued behind the trial)
    if (!cost_out && mf_trial(ctx, NLLS_VARS_CURRENT)) { defer_linearisation(ctx); return NLLS_OK; }
    // cost_out == NULL: the caller does not want the cost (the outer loop between iterations, src/optimize.jl:167-170
    // discards it) -- the sweep is then only enqueued: no partial-sum kernel, no synchronisation
    if (ctx->reduce_fn) {
        // collective (include/nlls_amd.h): this rank's blocks, then ONE sum over ranks of [cost | reduced rows of A.data | reduced part of b]
        const bool lazy = !cost_out && ctx->info.is_sparse && !ctx->elim_slab;
        if (ctx->phase_on && ctx->phase_ev.size() >= 8) {      // (the previous sweep's pair has long completed: the trials between synchronise)
            float ms = 0.f; if (ctx->phase_sweeps >= 0 && hipEventElapsedTime(&ms, ctx->phase_ev[6], ctx->phase_ev[7]) == hipSuccess) { ctx->phase_ms[5] += ms; ctx->phase_sweeps++; } else (void)hipGetLastError();
            (void)hipEventRecord(ctx->phase_ev[6], ctx->stream);
        }
        TRY(enqueue_sweep_gradhess(ctx, !lazy));
        if (ctx->phase_on && ctx->phase_ev.size() >= 8) (void)hipEventRecord(ctx->phase_ev[7], ctx->stream);
        new_linearisation(ctx, !lazy);
        if (lazy) return NLLS_OK;                                            // nothing is summed now: ensure_reduced_summed, or never
        if (ctx->nranks > 1) { ctx->n_stage0++; TRY(enqueue_pack_reduce0(ctx)); TRY(comm_reduce(ctx, ctx->redbuf.p, ctx->redbuf_len, NLLS_REDUCE_SUM)); TRY(enqueue_unpack_reduce0(ctx, true)); }
        else TRY(comm_reduce(ctx, ctx->scalars.p, 1, NLLS_REDUCE_SUM));      // (one rank through the route: the same number of collectives)
        if (!cost_out) return NLLS_OK;
        TRY(fetch_scalars(ctx, 0, 1)); *cost_out = ctx->h_scalars[0];
        return NLLS_OK;
    }
    // (where the matrix-free trial applies the cost is ITS sum of the blocks -- the one nlls_sweep_cost and every trial report: one fixed sum, bit for bit the same everywhere)
    const bool mfcost = cost_out && mf_trial(ctx, NLLS_VARS_CURRENT);
    TRY(enqueue_sweep_gradhess(ctx, cost_out != nullptr && !mfcost));
    if (mfcost) TRY(enqueue_mf_sweep_cost(ctx, NLLS_VARS_CURRENT));
    new_linearisation(ctx);
    if (!cost_out) return NLLS_OK;
    TRY(fetch_scalars(ctx, 0, 1));
    *cost_out = ctx->h_scalars[0];
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_sweep_cost(nlls_ctx* ctx, int32_t which, double* cost_out) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(which)) return NLLS_ERR_INVALID_ARG;
    // (where the matrix-free trial applies, every cost is ONE fixed sum -- the trial's: cost(problem) == result.bestcost bit for bit)
    if (mf_trial(ctx, NLLS_VARS_CURRENT)) TRY(enqueue_mf_sweep_cost(ctx, which)); else
    TRY(enqueue_sweep_cost(ctx, which));
    TRY(comm_reduce(ctx, ctx->scalars.p, 1, NLLS_REDUCE_SUM));       // (collective mode: the ranks' partial costs)
    TRY(fetch_scalars(ctx, 0, 1));
    if (cost_out) *cost_out = ctx->h_scalars[0];
    return NLLS_OK;
    NLLS_API_END(ctx)
}

// computeresidual / r'r / robustify / rho' of every block of one cost group, in upload order (nlls_eval.hip).  Reads only: no event of nlls_state.hpp.
int nlls_eval_blocks(nlls_ctx* ctx, int32_t which, int32_t group, double* r_out, double* sqerr_out, double* rho_out, double* weight_out) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(which)) return NLLS_ERR_INVALID_ARG;
    if (!r_out && !sqerr_out && !rho_out && !weight_out) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_eval_blocks: no output asked for");
    if (ctx->nranks > 1) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_eval_blocks under nlls_set_shard: a rank holds only its own cost blocks");
    if (group < 0 || group >= (int32_t)ctx->groups.size()) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_eval_blocks: bad cost group");
    const Group& G = ctx->groups[(size_t)group];
    if (G.res_kind == NLLS_COST_LINEAR3 || G.res_kind == NLLS_COST_DYN_LINEAR) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_eval_blocks: a non-squared cost kind has no residual");
    if (G.ncost == 0) return NLLS_OK;
    const size_t n = (size_t)G.ncost, nr = (size_t)eval_nres(G), need = n * (nr + 3);
    if (ctx->eval_out.n < need) HIP_TRY(ctx, ctx->eval_out.alloc(need));
    double* d_r = ctx->eval_out.p; double* d_sq = d_r + n * nr; double* d_rho = d_sq + n; double* d_w = d_rho + n;
    TRY(enqueue_eval_blocks(ctx, G, which, r_out ? d_r : nullptr, sqerr_out ? d_sq : nullptr, rho_out ? d_rho : nullptr, weight_out ? d_w : nullptr));
    if (r_out) HIP_TRY(ctx, hipMemcpyAsync(r_out, d_r, sizeof(double) * n * nr, hipMemcpyDeviceToHost, ctx->stream));
    if (sqerr_out) HIP_TRY(ctx, hipMemcpyAsync(sqerr_out, d_sq, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (rho_out) HIP_TRY(ctx, hipMemcpyAsync(rho_out, d_rho, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (weight_out) HIP_TRY(ctx, hipMemcpyAsync(weight_out, d_w, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// computeresjac / computecostgradhess of the listed blocks of one cost group, every slot free (nlls_linearize.hip).  Read only, like nlls_eval_blocks.
int nlls_eval_jacobians(nlls_ctx* ctx, int32_t which, int32_t group, int64_t n, const int64_t* index, double* r_out, double* J_out) { NLLS_API_BEGIN
    NEED_READY();
    double* const out[3] = {r_out, J_out, nullptr};
    return linearize_call(ctx, "nlls_eval_jacobians", which, group, n, index, true, out);
    NLLS_API_END(ctx)
}
int nlls_eval_gradhess(nlls_ctx* ctx, int32_t which, int32_t group, int64_t n, const int64_t* index, double* cost_out, double* g_out, double* H_out) { NLLS_API_BEGIN
    NEED_READY();
    double* const out[3] = {cost_out, g_out, H_out};
    return linearize_call(ctx, "nlls_eval_gradhess", which, group, n, index, false, out);
    NLLS_API_END(ctx)
}
// Matrix-free products with the linearisation (nlls_apply.hip).  These bodies validate, stage the caller's vectors in ApplyIndex::io, and synchronise; the launches are
// enqueue_hess_apply and its siblings, on device pointers.  Read only: no event of nlls_state.hpp.
int nlls_hess_apply(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* v, double* y_out) { NLLS_API_BEGIN
    if (!ctx || !v || !y_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    if (!valid_set(which) || nvec < 1 || nvec > NLLS_APPLY_MAX_VEC || !std::isfinite(lambda)) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_hess_apply: bad variable set, nvec or lambda");
    TRY(apply_check(ctx, "nlls_hess_apply", -1, false));
    const size_t nv = (size_t)nvec * (size_t)ctx->info.ndof;
    if (nv == 0) return NLLS_OK;
    double* io = nullptr; TRY(apply_io(ctx, 2 * nv, &io));
    HIP_TRY(ctx, hipMemcpyAsync(io, v, sizeof(double) * nv, hipMemcpyHostToDevice, ctx->stream));
    TRY(enqueue_hess_apply(ctx, which, lambda, nvec, io, io + nv));
    HIP_TRY(ctx, hipMemcpyAsync(y_out, io + nv, sizeof(double) * nv, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_jac_apply(nlls_ctx* ctx, int32_t which, int32_t group, int32_t nvec, const double* v, double* u_out) { NLLS_API_BEGIN
    if (!ctx || !v || !u_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    if (!valid_set(which) || nvec < 1 || nvec > NLLS_APPLY_MAX_VEC || group < 0 || group >= (int32_t)ctx->groups.size()) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_jac_apply: bad variable set, group or nvec");
    TRY(apply_check(ctx, "nlls_jac_apply", group, true));
    const Group& G = ctx->groups[(size_t)group];
    const size_t nv = (size_t)nvec * (size_t)ctx->info.ndof, nu = (size_t)nvec * (size_t)G.ncost * (size_t)G.nres;
    if (nv == 0 || nu == 0) return NLLS_OK;
    double* io = nullptr; TRY(apply_io(ctx, nv + nu, &io));
    HIP_TRY(ctx, hipMemcpyAsync(io, v, sizeof(double) * nv, hipMemcpyHostToDevice, ctx->stream));
    TRY(enqueue_jac_apply(ctx, which, group, nvec, io, io + nv));
    HIP_TRY(ctx, hipMemcpyAsync(u_out, io + nv, sizeof(double) * nu, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_jact_apply(nlls_ctx* ctx, int32_t which, int32_t group, int32_t nvec, const double* u, double* y_out) { NLLS_API_BEGIN
    if (!ctx || !u || !y_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    if (!valid_set(which) || nvec < 1 || nvec > NLLS_APPLY_MAX_VEC || group < 0 || group >= (int32_t)ctx->groups.size()) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_jact_apply: bad variable set, group or nvec");
    TRY(apply_check(ctx, "nlls_jact_apply", group, true));
    const Group& G = ctx->groups[(size_t)group];
    const size_t nv = (size_t)nvec * (size_t)ctx->info.ndof, nu = (size_t)nvec * (size_t)G.ncost * (size_t)G.nres;
    if (nv == 0) return NLLS_OK;
    double* io = nullptr; TRY(apply_io(ctx, nv + nu, &io));
    if (nu) HIP_TRY(ctx, hipMemcpyAsync(io, u, sizeof(double) * nu, hipMemcpyHostToDevice, ctx->stream));
    TRY(enqueue_jact_apply(ctx, which, group, nvec, io, io + nu));
    HIP_TRY(ctx, hipMemcpyAsync(y_out, io + nu, sizeof(double) * nv, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_hess_block_diag(nlls_ctx* ctx, int32_t which, double lambda, double* d_out) { NLLS_API_BEGIN
    if (!ctx || !d_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    if (!valid_set(which) || !std::isfinite(lambda)) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_hess_block_diag: bad variable set or lambda");
    TRY(apply_check(ctx, "nlls_hess_block_diag", -1, false));
    const size_t nd = (size_t)apply_diag_len(ctx);
    if (nd == 0) return NLLS_OK;
    double* io = nullptr; TRY(apply_io(ctx, nd, &io));
    TRY(enqueue_hess_block_diag(ctx, which, lambda, io));
    HIP_TRY(ctx, hipMemcpyAsync(d_out, io, sizeof(double) * nd, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// optimize(kernel::ContaminatedGaussian, squarederrors, maxiters)  src/robustadaptive.jl:48-73 on the device (nlls_eval.hip): one synchronisation
int nlls_adaptive_em(nlls_ctx* ctx, int32_t which, int64_t kernel_var, int32_t maxiters, double storage_out[3], int32_t* iters_out) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(which) || maxiters < 0) return NLLS_ERR_INVALID_ARG;
    if (ctx->nranks > 1) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_adaptive_em under nlls_set_shard: a rank holds only its own cost blocks");
    const int64_t v = kernel_var - 1;
    if (v < 0 || v >= ctx->info.nvar || ctx->var_kind[(size_t)v] != NLLS_VAR_CONTAMINATED_GAUSSIAN) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_adaptive_em: kernel_var is not a NLLS_VAR_CONTAMINATED_GAUSSIAN variable");
    if (!std::binary_search(ctx->em_kernel_vars.begin(), ctx->em_kernel_vars.end(), v)) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_adaptive_em: no block of an adaptive kind has this variable as its kernel");
    // writing the set: the transition nlls_set_variables(which) makes (what it enqueues goes ahead of the passes, in stream order)
    if (maxiters > 0) { TRY(vars_written(ctx, which)); if (which == NLLS_VARS_CURRENT) { new_starting_point(ctx); ctx->tb_prev_end = 0.0; } }
    TRY(enqueue_adaptive_em(ctx, which, ctx->var_off[(size_t)v], maxiters));
    double st[10];
    HIP_TRY(ctx, hipMemcpyAsync(st, ctx->em_state.p, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (storage_out) { storage_out[0] = st[0]; storage_out[1] = st[1]; storage_out[2] = st[2]; }
    if (iters_out) *iters_out = (int32_t)st[8];
    return NLLS_OK;
    NLLS_API_END(ctx)
}

// The cost blocks' payload and a group's robust parameters replaced on the uploaded structure (nlls_update.hip; the reference's mutable costs, src/optimize.jl:5-17).
// Everything is checked on the host before anything is enqueued or any state changes.
int nlls_set_cost_data(nlls_ctx* ctx, int32_t group, int64_t n, const int64_t* index, const double* data) { NLLS_API_BEGIN
    NEED_READY();
    if (ctx->shard_nranks > 1) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_set_cost_data under nlls_set_shard: a rank holds only its own cost blocks");
    if (group < 0 || group >= (int32_t)ctx->groups.size()) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_cost_data: bad cost group");
    Group& G = ctx->groups[(size_t)group];
    if (n < 0 || n > G.ncost) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_cost_data: n outside 0 .. ncost");
    if (n == 0) return NLLS_OK;
    if (!data) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_cost_data: data is NULL");
    std::vector<uint32_t> blocks;                       // the listed blocks, 0-based, as the device takes them
    if (index) { std::vector<uint8_t> seen((size_t)G.ncost, 0); blocks.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) { const int64_t k = index[i] - 1;
            if (k < 0 || k >= G.ncost) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_cost_data: index outside 1 .. ncost");
            if (seen[(size_t)k]) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_cost_data: a block is listed twice");
            seen[(size_t)k] = 1; blocks[(size_t)i] = (uint32_t)k; } }
    if (G.ndata <= 0) return NLLS_OK;                   // (a kind without payload: nothing to write, nothing changed)
    const size_t nd = (size_t)n * (size_t)G.ndata;
    if (ctx->upd_stage.n < nd) HIP_TRY(ctx, ctx->upd_stage.alloc(nd));
    if (index && ctx->upd_index.n < (size_t)n) HIP_TRY(ctx, ctx->upd_index.alloc((size_t)n));
    costs_changed(ctx); ctx->tb_prev_end = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->upd_stage.p, data, sizeof(double) * nd, hipMemcpyHostToDevice, ctx->stream));
    if (index) HIP_TRY(ctx, hipMemcpyAsync(ctx->upd_index.p, blocks.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (the caller's buffers are read during the call only; the scatter itself is left enqueued)
    return enqueue_update_scatter(ctx, G, n, index != nullptr);
    NLLS_API_END(ctx)
}
int nlls_set_robust_params(nlls_ctx* ctx, int32_t group, const double params[4]) { NLLS_API_BEGIN
    NEED_READY();
    if (ctx->shard_nranks > 1) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_set_robust_params under nlls_set_shard");
    if (group < 0 || group >= (int32_t)ctx->groups.size() || !params) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_robust_params: bad cost group or NULL parameters");
    Group& G = ctx->groups[(size_t)group];
    if (G.adaptive) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_robust_params: the kernel of an adaptive group is a variable");
    // Group::rk is the one copy: every launch takes it by value (sweeps, trials, nlls_eval_blocks; nlls_optimize_singles fills its group table per call)
    G.rk.p0 = params[0]; G.rk.p1 = params[1]; G.rk.p2 = params[2];
    costs_changed(ctx); ctx->tb_prev_end = 0.0;
    return NLLS_OK;
    NLLS_API_END(ctx)
}

int nlls_get_grad(nlls_ctx* ctx, double* b_out) { NLLS_API_BEGIN
    NEED_GRAD(); if (!b_out) return NLLS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(b_out, ctx->b.p, sizeof(double) * ctx->info.ndof, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_get_bsm_data(nlls_ctx* ctx, double* data_out) { NLLS_API_BEGIN
    NEED_GRAD(); if (!data_out) return NLLS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(data_out, ctx->A.p, sizeof(double) * ctx->info.nnz_data, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_max_abs_diag(nlls_ctx* ctx, double* out) { NLLS_API_BEGIN
    NEED_GRAD(); TRY(enqueue_max_abs_diag(ctx)); TRY(comm_reduce(ctx, ctx->scalars.p + 3, 1, NLLS_REDUCE_MAX)); TRY(fetch_scalars(ctx, 3, 1));
    if (out) *out = ctx->h_scalars[3]; return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_grad_sqnorm(nlls_ctx* ctx, double* out) { NLLS_API_BEGIN
    NEED_GRAD(); TRY(enqueue_quadform(ctx, ctx->b.p, 6)); TRY(comm_reduce(ctx, ctx->scalars.p + 6, 2, NLLS_REDUCE_SUM)); TRY(fetch_scalars(ctx, 6, 2));
    if (out) *out = ctx->h_scalars[7]; return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_grad_quadform(nlls_ctx* ctx, double* out) { NLLS_API_BEGIN
    NEED_GRAD(); TRY(enqueue_quadform(ctx, ctx->b.p, 6)); TRY(comm_reduce(ctx, ctx->scalars.p + 6, 2, NLLS_REDUCE_SUM)); TRY(fetch_scalars(ctx, 6, 2));
    if (out) *out = ctx->h_scalars[6]; return NLLS_OK;
    NLLS_API_END(ctx)
}

// what a non-zero factorisation status means: a bad pivot (NLLS_ERR_NOT_SPD: the iterators damp more and retry) or a hand-off inside a one-launch backward pass that
// timed out (0x40000000, nlls_bcr.hip: not a property of the system -- NLLS_ERR_HIP; NLLS_BCR_LEVEL_BACKWARD=1 / NLLS_DENSE_STEP_BACKWARD=1 select the per-level launches)
static int status_error(nlls_ctx* ctx, int32_t st, const char* what) {
    if (st == 0x40000000) return fail(ctx, NLLS_ERR_HIP, "a hand-off between workgroups of the one-launch backward substitution timed out (0.5 s): not a pivot failure -- NLLS_BCR_LEVEL_BACKWARD=1 / NLLS_DENSE_STEP_BACKWARD=1 select the per-level launches");
    return fail(ctx, NLLS_ERR_NOT_SPD, std::string(what) + " (code " + std::to_string(st) + ")");
}
int nlls_damp(nlls_ctx* ctx, double delta) { NLLS_API_BEGIN NEED_GRAD_LAZY(); ctx->lambda += delta; return NLLS_OK; NLLS_API_END(ctx) }

int nlls_solve(nlls_ctx* ctx, double* x_out) { NLLS_API_BEGIN
    NEED_GRAD();
    TRY(enqueue_solve(ctx));
    // what the iterators ask about the step next -- max |x|, |x|, x'Hx, g'x (src/optimize.jl:149, src/iterators.jl:160-163) --
    // is computed behind the solve and comes back with the same synchronisation; the queries then answer from the host
    drop(ctx->step.cached);
    const bool precompute = ctx->nranks == 1;
    if (precompute) { TRY(enqueue_post_solve(ctx, ctx->stamp_ptr())); }
    int32_t status[4] = {0, 0, 0, 0};
    if (precompute) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars + 1, ctx->scalars.p + 1, sizeof(double) * 10, hipMemcpyDeviceToHost, ctx->stream));   // ... and the status in [10]
    else HIP_TRY(ctx, hipMemcpyAsync(status, ctx->d_status.p, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
    if (x_out) HIP_TRY(ctx, hipMemcpyAsync(x_out, ctx->x.p, sizeof(double) * ctx->info.ndof, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (precompute) { status[0] = (int32_t)ctx->h_scalars[10]; step_solved(ctx, false); }
    if (status[0] != 0) return status_error(ctx, status[0], "factorisation met a non-positive pivot");
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// The iteration's own arguments: the one condition of nlls_solve_pcg, nlls_solve_pcg_rhs and nlls_marginal_cov
static bool pcg_iteration_args_ok(int32_t precond, int32_t maxiters, double rtol, bool reduced = false) {
    return (precond == NLLS_PCG_PRECOND_NONE || precond == NLLS_PCG_PRECOND_BLOCK_JACOBI || (reduced && precond == NLLS_PCG_PRECOND_SCHUR_JACOBI)) && maxiters >= 1 && std::isfinite(rtol) && rtol >= 0;
}
// NLLS_PCG_PRECOND_SCHUR_JACOBI where there is no reduced system: refused like any bad preconditioner, and the text says where it belongs
static std::string pcg_bad_args(const char* name, int32_t precond, const char* what) {
    if (precond == NLLS_PCG_PRECOND_SCHUR_JACOBI) return std::string(name) + ": NLLS_PCG_PRECOND_SCHUR_JACOBI belongs to the reduced system: it preconditions nlls_solve_pcg_schur only";
    return std::string(name) + ": bad " + what;
}
// The same solve by conjugate gradients on the matrix-free operator (nlls_pcg.hip): (H + lambda I) y = b from y = 0, x = -y.  Everything is refused here, before anything is
// enqueued; the solver's rounds synchronise.  On success the transition nlls_set_step makes (step_replaced, inside pcg_solve); a breakdown leaves x as it was.
int nlls_solve_pcg(nlls_ctx* ctx, int32_t precond, int32_t maxiters, double rtol, double* x_out, double* stats_out) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    if (!pcg_iteration_args_ok(precond, maxiters, rtol)) return fail(ctx, NLLS_ERR_INVALID_ARG, pcg_bad_args("nlls_solve_pcg", precond, "preconditioner, maxiters or rtol"));
    NEED_GRAD_LAZY();
    TRY(apply_check(ctx, "nlls_solve_pcg", -1, false));
    if (ctx->info.ndof == 0) { ctx->pcg_iters = ctx->pcg_status = ctx->pcg_rounds = 0; if (stats_out) for (int k = 0; k < 8; ++k) stats_out[k] = 0.0; return NLLS_OK; }
    TRY(ensure_grad(ctx, 2)); TRY(ensure_reduced_summed(ctx));      // (b as nlls_get_grad reads it)
    return pcg_solve(ctx, precond, maxiters, rtol, x_out, stats_out);
    NLLS_API_END(ctx)
}
// Conjugate gradients on right-hand sides of the caller's, and on unit columns for a block of the inverse (nlls_pcg.hip, pcg_solve_cols).  Read only, like the products:
// no event of nlls_state.hpp, nothing of the last nlls_solve_pcg's counters.  Everything is refused here, before anything is enqueued or written.
static int pcg_cols_check(nlls_ctx* ctx, const char* name, int32_t which, double lambda, int32_t precond, int32_t maxiters, double rtol) {
    if (!valid_set(which) || !std::isfinite(lambda) || !pcg_iteration_args_ok(precond, maxiters, rtol))
        return fail(ctx, NLLS_ERR_INVALID_ARG, pcg_bad_args(name, precond, "variable set, lambda, preconditioner, maxiters or rtol"));
    return NLLS_OK;
}
int nlls_solve_pcg_rhs(nlls_ctx* ctx, int32_t which, double lambda, int32_t precond, int32_t maxiters, double rtol, int32_t nrhs, const double* B, double* X_out, double* stats_out) { NLLS_API_BEGIN
    if (!ctx || !B || !X_out) return NLLS_ERR_INVALID_ARG;
    if (nrhs < 1) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_solve_pcg_rhs: nrhs < 1");
    TRY(pcg_cols_check(ctx, "nlls_solve_pcg_rhs", which, lambda, precond, maxiters, rtol));
    NEED_READY();
    TRY(apply_check(ctx, "nlls_solve_pcg_rhs", -1, false));
    if (ctx->info.ndof == 0) { if (stats_out) for (int64_t k = 0; k < 4 * (int64_t)nrhs + 4; ++k) stats_out[k] = 0.0; return NLLS_OK; }
    return pcg_solve_cols(ctx, PcgCall{.name = "nlls_solve_pcg_rhs", .which = which, .lambda = lambda, .precond = precond, .maxiters = maxiters, .rtol = rtol, .ncols = nrhs, .B = B, .out = X_out}, stats_out);
    NLLS_API_END(ctx)
}
int nlls_marginal_cov(nlls_ctx* ctx, int32_t which, double lambda, int64_t nsel, const int64_t* varindices, int32_t precond, int32_t maxiters, double rtol, double* cov_out, double* stats_out) { NLLS_API_BEGIN
    if (!ctx || !varindices || !cov_out) return NLLS_ERR_INVALID_ARG;
    if (nsel < 1) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_marginal_cov: nsel < 1");
    TRY(pcg_cols_check(ctx, "nlls_marginal_cov", which, lambda, precond, maxiters, rtol));
    NEED_READY();
    TRY(apply_check(ctx, "nlls_marginal_cov", -1, false));
    std::vector<int64_t> rows; std::vector<uint8_t> seen((size_t)ctx->info.nvar, 0);      // the unknowns of the listed variables, in the listed order
    for (int64_t i = 0; i < nsel; ++i) { const int64_t v = varindices[i] - 1;
        if (v < 0 || v >= ctx->info.nvar) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_marginal_cov: a variable index outside 1 .. nvar");
        if (seen[(size_t)v]) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_marginal_cov: a variable is listed twice");
        seen[(size_t)v] = 1;
        const uint64_t blk = ctx->blockindices[(size_t)v];
        if (blk == 0) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_marginal_cov: a listed variable is fixed: it has no row in H");
        for (int32_t k = 0; k < ctx->blocksizes[(size_t)(blk - 1)]; ++k) rows.push_back(ctx->boffsets[(size_t)(blk - 1)] + k); }
    const int64_t m = (int64_t)rows.size();
    if (m == 0) { if (stats_out) for (int k = 0; k < 4; ++k) stats_out[k] = 0.0; return NLLS_OK; }
    return pcg_solve_cols(ctx, PcgCall{.name = "nlls_marginal_cov", .which = which, .lambda = lambda, .precond = precond, .maxiters = maxiters, .rtol = rtol, .ncols = m, .rows = rows.data(), .out = cov_out}, stats_out);
    NLLS_API_END(ctx)
}
// ---- the reduced system, matrix-free (nlls_schur_apply.hip) ------------------------------------------------------------------------------------------
// The three products: everything is refused before anything is built or enqueued; then the r/e index, the caller's vectors into SchurIndex::io, the e blocks' inverses,
// the product; the factor's status comes home first, and only a call whose blocks all have a factor copies a result out.  Read only: no event of nlls_state.hpp.
static int schur_product(nlls_ctx* ctx, const char* name, int mode, int32_t which, double lambda, int32_t nvec, const double* a, const double* yr, double* out) {
    const std::string nm(name);
    if (!valid_set(which) || nvec < 1 || nvec > NLLS_APPLY_MAX_VEC || !std::isfinite(lambda)) return fail(ctx, NLLS_ERR_INVALID_ARG, nm + ": bad variable set, nvec or lambda");
    TRY(schur_check(ctx, name));
    TRY(schur_prepare(ctx));
    SchurIndex& Z = ctx->sch;
    const size_t nf = (size_t)nvec * (size_t)ctx->info.ndof, nr = (size_t)nvec * (size_t)Z.nred;
    const size_t na = mode == SCHUR_APPLY ? nr : nf, ny = mode == SCHUR_EXPAND ? nr : 0, no = mode == SCHUR_EXPAND ? nf : nr, nd = (size_t)std::max<int64_t>(apply_diag_len(ctx), 1);
    if (no == 0) return NLLS_OK;            // (every unfixed block eliminated: a reduced vector has no entry, nlls_schur_apply and nlls_schur_reduce have nothing to write)
    auto need = [&](DevBuf<double>& buf, size_t n, const char* what) -> int {
        if (buf.n >= n && buf.p) return NLLS_OK;
        const hipError_t e = buf.alloc(n); if (e != hipSuccess) { buf.release(); (void)hipGetLastError(); return hip_fail(ctx, e, (nm + ": " + what).c_str()); }
        return NLLS_OK; };
    TRY(need(Z.io, std::max<size_t>(na + ny + no, 1), "staging for the vectors")); TRY(need(Z.Cinv, nd, "the eliminated blocks' inverses")); TRY(need(Z.scal, PCG_NSCAL, "the factor's status"));
    double* const io = Z.io.p; double st[PCG_NSCAL] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(ctx, hipMemsetAsync(Z.scal.p, 0, sizeof(double) * PCG_NSCAL, ctx->stream));
    if (na) HIP_TRY(ctx, hipMemcpyAsync(io, a, sizeof(double) * na, hipMemcpyHostToDevice, ctx->stream));
    if (ny) HIP_TRY(ctx, hipMemcpyAsync(io + na, yr, sizeof(double) * ny, hipMemcpyHostToDevice, ctx->stream));
    TRY(enqueue_schur_setup(ctx, which, lambda, SCHUR_R_NONE, Z.Cinv.p, Z.scal.p, nullptr));
    TRY(enqueue_schur_op(ctx, mode, which, lambda, Z.Cinv.p, nvec, io, io + na, io + na + ny));
    HIP_TRY(ctx, hipMemcpyAsync(st, Z.scal.p, sizeof(double) * PCG_NSCAL, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (st[PCG_STATUS] != 0.0) return fail(ctx, NLLS_ERR_NOT_SPD, nm + ": an eliminated block C_e + lambda I is not positive definite");
    if (no) HIP_TRY(ctx, hipMemcpyAsync(out, io + na + ny, sizeof(double) * no, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
}
int nlls_schur_info(const nlls_ctx* ctx, int64_t* nred_out, int64_t* nelim_out, uint8_t* is_elim_out) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    if (!ctx->ready) return NLLS_ERR_NOT_READY;
    const size_t nb = ctx->blocksizes.size(); const bool have = ctx->is_elim.size() == nb;
    int64_t nred = 0, nelim = 0;
    for (size_t b = 0; b < nb; ++b) { const bool e = have && ctx->is_elim[b]; if (e) ++nelim; else nred += ctx->blocksizes[b]; if (is_elim_out) is_elim_out[b] = e ? 1 : 0; }
    if (nred_out) *nred_out = nred;
    if (nelim_out) *nelim_out = nelim;
    return NLLS_OK;
    NLLS_API_END(const_cast<nlls_ctx*>(ctx))
}
int nlls_schur_apply(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* v, double* y_out) { NLLS_API_BEGIN
    if (!ctx || !v || !y_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    return schur_product(ctx, "nlls_schur_apply", SCHUR_APPLY, which, lambda, nvec, v, nullptr, y_out);
    NLLS_API_END(ctx)
}
int nlls_schur_reduce(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* b, double* s_out) { NLLS_API_BEGIN
    if (!ctx || !b || !s_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    return schur_product(ctx, "nlls_schur_reduce", SCHUR_REDUCE, which, lambda, nvec, b, nullptr, s_out);
    NLLS_API_END(ctx)
}
int nlls_schur_expand(nlls_ctx* ctx, int32_t which, double lambda, int32_t nvec, const double* b, const double* yr, double* y_out) { NLLS_API_BEGIN
    if (!ctx || !b || !yr || !y_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    return schur_product(ctx, "nlls_schur_expand", SCHUR_EXPAND, which, lambda, nvec, b, yr, y_out);
    NLLS_API_END(ctx)
}
// The diagonal blocks of S(lambda), unfactored (nlls_schur_apply.hip, enqueue_schur_setup under SCHUR_R_S): the rules of the products -- refused before anything is built
// or enqueued, the e factor's status home before a byte is copied out, read only.  The set-up is no product: the products' statistics (nlls_get_solve_stats [47..50])
// keep describing the last product.
int nlls_schur_block_diag(nlls_ctx* ctx, int32_t which, double lambda, double* d_out) { NLLS_API_BEGIN
    if (!ctx || !d_out) return NLLS_ERR_INVALID_ARG;
    NEED_READY();
    if (!valid_set(which) || !std::isfinite(lambda)) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_schur_block_diag: bad variable set or lambda");
    TRY(schur_check(ctx, "nlls_schur_block_diag"));
    TRY(schur_prepare(ctx));
    SchurIndex& Z = ctx->sch;
    if (Z.nred == 0) return NLLS_OK;        // (every unfixed block eliminated: there is no reduced block)
    size_t no = 0; for (size_t b = 0; b < ctx->blocksizes.size(); ++b) if (!ctx->is_elim[b]) no += (size_t)ctx->blocksizes[b] * (size_t)ctx->blocksizes[b];
    auto need = [&](DevBuf<double>& buf, size_t n, const char* what) -> int {
        if (buf.n >= n && buf.p) return NLLS_OK;
        const hipError_t e = buf.alloc(n); if (e != hipSuccess) { buf.release(); (void)hipGetLastError(); return hip_fail(ctx, e, (std::string("nlls_schur_block_diag: ") + what).c_str()); }
        return NLLS_OK; };
    TRY(need(Z.io, std::max<size_t>(no, 1), "staging for the blocks")); TRY(need(Z.Cinv, (size_t)std::max<int64_t>(apply_diag_len(ctx), 1), "the eliminated blocks' inverses")); TRY(need(Z.scal, PCG_NSCAL, "the factor's status"));
    double st[PCG_NSCAL] = {0, 0, 0, 0, 0, 0, 0, 0}; const int64_t scratch = ctx->app_scratch;
    HIP_TRY(ctx, hipMemsetAsync(Z.scal.p, 0, sizeof(double) * PCG_NSCAL, ctx->stream));
    const int rc = enqueue_schur_setup(ctx, which, lambda, SCHUR_R_S, Z.Cinv.p, Z.scal.p, nullptr, Z.io.p);
    ctx->app_scratch = scratch;
    TRY(rc);
    HIP_TRY(ctx, hipMemcpyAsync(st, Z.scal.p, sizeof(double) * PCG_NSCAL, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (st[PCG_STATUS] != 0.0) return fail(ctx, NLLS_ERR_NOT_SPD, "nlls_schur_block_diag: an eliminated block C_e + lambda I is not positive definite");
    HIP_TRY(ctx, hipMemcpyAsync(d_out, Z.io.p, sizeof(double) * no, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// nlls_solve_pcg on the reduced system: refused as it refuses, and where nothing was eliminated; the transition nlls_set_step makes on success (inside pcg_solve_schur)
int nlls_solve_pcg_schur(nlls_ctx* ctx, int32_t precond, int32_t maxiters, double rtol, double* x_out, double* stats_out) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    if (!pcg_iteration_args_ok(precond, maxiters, rtol, /*reduced=*/true)) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_solve_pcg_schur: bad preconditioner, maxiters or rtol");
    NEED_GRAD_LAZY();
    TRY(schur_check(ctx, "nlls_solve_pcg_schur"));
    TRY(ensure_grad(ctx, 2)); TRY(ensure_reduced_summed(ctx));      // (b as nlls_get_grad reads it)
    return pcg_solve_schur(ctx, precond, maxiters, rtol, x_out, stats_out);
    NLLS_API_END(ctx)
}
// nlls_solve_pcg inside a trust region (Steihaug-Toint; nlls_pcg.hip, pcg_solve_tr): refused as it refuses, and for a radius that is no radius; +inf is one
int nlls_solve_pcg_tr(nlls_ctx* ctx, int32_t precond, int32_t maxiters, double rtol, double radius, double* x_out, double* stats_out) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    if (!pcg_iteration_args_ok(precond, maxiters, rtol) || !(radius > 0.0)) return fail(ctx, NLLS_ERR_INVALID_ARG, pcg_bad_args("nlls_solve_pcg_tr", precond, "preconditioner, maxiters, rtol or radius"));
    NEED_GRAD_LAZY();
    TRY(apply_check(ctx, "nlls_solve_pcg_tr", -1, false));
    if (ctx->info.ndof == 0) { if (stats_out) for (int k = 0; k < 8; ++k) stats_out[k] = 0.0; return NLLS_OK; }
    TRY(ensure_grad(ctx, 2)); TRY(ensure_reduced_summed(ctx));      // (b as nlls_get_grad reads it)
    return pcg_solve_tr(ctx, precond, maxiters, rtol, radius, x_out, stats_out);
    NLLS_API_END(ctx)
}
// One Levenberg-Marquardt trial in one call and one synchronisation (src/iterators.jl:149-157): uniformscaling!(H, dlambda),
// solve!, negate!, update!(to, from, x), cost(to).  Same kernels, same order as the separate entry points.
int nlls_lm_trial(nlls_ctx* ctx, double dlambda, int32_t to, int32_t from, double* cost_out) { NLLS_API_BEGIN
    NEED_GRAD_LAZY(); if (!valid_set(to) || !valid_set(from) || to == from) return NLLS_ERR_INVALID_ARG;
    const bool mf = mf_trial(ctx, from);           // matrix-free: the eliminated rows of A.data are neither needed nor formed (nlls_mf.hip)
    TRY(ensure_grad(ctx, mf ? 1 : 2));             // (a trial right behind a REJECTED one: the look-ahead sweep of that trial's point is in A and b)
    const bool collective = ctx->reduce_fn != nullptr && ctx->info.is_sparse && !ctx->replicated;
    if (!collective) TRY(ensure_reduced_summed(ctx));
    if (ctx->nranks != 1 && !collective) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_lm_trial under nlls_set_shard needs an all-reduce (nlls_comm_init_rccl / nlls_set_allreduce), or the *_local / *_finish pairs");
    ctx->lambda += dlambda;
    drop(ctx->step.cached);
    if (collective) {
        // the sharded trial, end to end on this rank's stream: local elimination, ONE sum of [S | s] over ranks, the reduced system solved on
        // every rank (each then holds the reduced part of the step: x is never summed), own back-substitution, retraction, own cost blocks,
        // and one gather of the ranks' scalars -- combined on the device and published to the host mirror as the single-GPU trial does
        if (ctx->nranks > 1 && !ctx->lin.summed) ctx->n_lazy_trials++;
        phase_mark(ctx, 0);
        TRY(enqueue_solve_local(ctx));
        phase_mark(ctx, 1);
        if (ctx->solve_mode == SOLVE_TSPARSE && ctx->tsp.nslots_assembled < ctx->tsp.nslots) {
            // tile-sparse layout [assembled tiles | fill tiles | strips | s]: the fill tiles and the strips are zero on every rank until the factorisation -- the assembled
            // prefix and s are what is summed (two collectives: on the 100 x 100 camera grid most of the volume was zeros)
            TRY(comm_reduce(ctx, ctx->S.p, ctx->tsp.nslots_assembled * (int64_t)TSP_TE, NLLS_REDUCE_SUM));
            TRY(comm_reduce(ctx, ctx->S.p + ctx->s_elems, ctx->nred, NLLS_REDUCE_SUM));
        } else TRY(comm_reduce(ctx, ctx->S.p, (int64_t)ctx->s_elems + ctx->nred, NLLS_REDUCE_SUM));
        phase_mark(ctx, 2);
        // (one rank through the route: the same launches as the unsharded trial; no mirror: the host waits on the gathered scalars, not on this rank's)
        const TrialArgs t{.to = to, .from = from, .replicate_xr = true};
        TRY(enqueue_solve_finish(ctx, t));
        phase_mark(ctx, 4);
        TRY(enqueue_lm_trial_tail(ctx, t));
        TRY(comm_gather_trial_scalars(ctx, (double)ctx->trial_seq));
        phase_mark(ctx, 5);
    } else if (ctx->tiny_dense) {
        const bool la = ctx->sw.spec_on && ctx->ahead.armed && from == NLLS_VARS_CURRENT;
        TRY(enqueue_tiny_dense_trial(ctx, to, from));
        if (la) TRY(enqueue_lookahead(ctx, to, 0));
        TRY(enqueue_tiny_trial_finish_pending(ctx));      // (the finishing reduction, unless the look-ahead sweep's accumulate launch took it along)
    } else {
    { double* st = ctx->h_scalars + 40; st[0] = st[1] = st[2] = st[3] = 0.0; }       // (the launches of this trial stamp them: device-timed buckets)
    TrialArgs t{.to = to, .from = from, .mf = mf, .mirror = ctx->h_scalars_dev}; ctx->mf_trials += mf;    // (the back-substitution launch may take the retraction with it)
    TRY(enqueue_solve(ctx, t));
    const bool la = ctx->sw.spec_on && ctx->ahead.armed && ctx->nranks == 1 && ctx->info.is_sparse && from == NLLS_VARS_CURRENT;
    // (matrix-free trial with a look-ahead sweep behind it: the trial's finishing workgroup rides in that sweep's launch -- nlls_sweep.hip -- unless rows have to be zeroed in between)
    t.zero_for_lookahead = la; t.defer_fin = mf && la && ctx->nzero == 0;
    drop(ctx->zero.heavy_rows); drop(ctx->fin.mf_pending);   // (left over only by a trial that failed in between)
    TRY(enqueue_lm_trial_tail(ctx, t));            // step statistics + quadratic form (+ retraction) and the cost sweep, one finishing launch
    if (la) TRY(enqueue_lookahead(ctx, to, mf ? 1 : 0));
    if (take(ctx->fin.mf_pending)) TRY(enqueue_mf_trial_finish_now(ctx, t));      // (no launch of the sweep took the finishing workgroup along)
    }
    // (sparse systems: the finishing launch -- TrialArgs::mirror, or comm_gather_trial_scalars -- has written the scalars, in [10] the status, to the pinned host mirror)
    if ((!ctx->info.is_sparse && !ctx->tiny_dense) || !ctx->h_scalars_dev) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->scalars.p, sizeof(double) * 12, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        // spin on the sequence numbers the finishing launch publishes (a few milliseconds at most: then fall back to the synchronisation,
        // after which the values are there in any case)
        volatile double* hs = ctx->h_scalars; const double seq = (double)ctx->trial_seq;
        const auto t0 = std::chrono::steady_clock::now(); bool seen = false;
        for (uint64_t spin = 0;; ++spin) {
            if (hs[32] == seq && hs[33] == seq) { seen = true; break; }
            // (a trial of the problems this path is built for ends within a millisecond; a long one sleeps in the synchronisation instead of
            //  burning a core)
            if ((spin & 255) == 255) { if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1500)) break; __builtin_ia32_pause(); }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (!seen) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    {   // device-timed buckets (nlls_ctx::tb_*): only a trial whose launches all stamped (the sparse single-GPU routes) counts
        const double* st = ctx->h_scalars + 40;
        if (!collective && st[0] > 0.0 && st[2] >= st[0] && st[3] >= st[2]) {
            const double k = ctx->tb_ns_per_tick;
            ctx->tb_solver_ns += (int64_t)((st[2] - st[0]) * k); ctx->tb_cost_ns += (int64_t)((st[3] - st[2]) * k); ctx->tb_trials++;
            if (ctx->tb_prev_end > 0.0 && st[0] >= ctx->tb_prev_end) ctx->tb_grad_ns += (int64_t)((st[0] - ctx->tb_prev_end) * k);
            ctx->tb_prev_end = st[3];
        }
    }
    if (collective && ctx->phase_on && ctx->phase_ev.size() >= 6) {      // (the trial has ended: every event has completed)
        if (hipEventSynchronize(ctx->phase_ev[5]) == hipSuccess) {
            float ms = 0.f; bool ok = true; double d[5];
            for (int k = 0; k < 5 && ok; ++k) { ok = hipEventElapsedTime(&ms, ctx->phase_ev[k], ctx->phase_ev[k + 1]) == hipSuccess; d[k] = ms; }
            if (ok) { for (int k = 0; k < 5; ++k) ctx->phase_ms[k] += d[k]; ctx->phase_trials++; } else (void)hipGetLastError();
        }
    }
    const int32_t status[1] = {(int32_t)ctx->h_scalars[10]};
    ctx->comm_gathered = collective;
    if (collective) ctx->comm_agreed = ctx->h_scalars[11];      // the ranks' posted termination flags, combined by maximum in the same gather (nlls_comm_agreed_flag)
    step_solved(ctx, true);
    if (status[0] != 0) return status_error(ctx, status[0], "factorisation met a non-positive pivot");
    if (cost_out) *cost_out = ctx->h_scalars[0];
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// The part of one Levenberg-Marquardt trial that follows the solve (src/iterators.jl:155-163), for sharded runs: with the
// step x complete on this rank (after the stage-2 reduction) -- update!(to, from, x), cost(to), fast_bAb(H, x), dot(g, x),
// maximum(abs, x), |x|^2 -- in one enqueue and one synchronisation.  out = [cost, x'Hx, g'x, max|x|, |x|^2]; under
// nlls_set_shard the first three are this rank's PARTIAL sums (the caller adds them over ranks), the last two are global.
int nlls_trial_local(nlls_ctx* ctx, int32_t to, int32_t from, double* out) { NLLS_API_BEGIN
    NEED_GRAD(); if (!valid_set(to) || !valid_set(from) || to == from) return NLLS_ERR_INVALID_ARG;
    TRY(enqueue_lm_trial_tail(ctx, TrialArgs{.to = to, .from = from, .mirror = ctx->h_scalars_dev}));     // step statistics + quadratic form + retraction in one launch, the cost sweep, one finishing launch
    if (!out) return NLLS_OK;                      // enqueue only: the eleven scalars stay on the device (reduce buffer 3) for a device-side gather
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_scalars, ctx->scalars.p, sizeof(double) * 11, hipMemcpyDeviceToHost, ctx->stream));   // [10]: the factorisation status
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    out[0] = ctx->h_scalars[0]; out[1] = ctx->h_scalars[8]; out[2] = ctx->h_scalars[5]; out[3] = ctx->h_scalars[1]; out[4] = ctx->h_scalars[2];
    if (ctx->nranks > 1) {
        // sharded: max|x| and |x|^2 over THIS rank's share of the step (its own eliminated blocks; rank 0 also the reduced part), and the
        // factorisation status as a sixth value instead of an error -- a rank-local zero pivot must not leave this rank out of the
        // collective its peers are about to enter: the caller reduces all six and raises on every rank
        out[4] = ctx->h_scalars[9]; out[5] = ctx->h_scalars[10];
        return NLLS_OK;
    }
    if ((int32_t)ctx->h_scalars[10] != 0) return status_error(ctx, (int32_t)ctx->h_scalars[10], "factorisation met a zero pivot");
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// nlls_solve_finish_async for a sharded LM trial: the reduced part of the step stays on every rank (no stage-2 reduction afterwards)
int nlls_solve_finish_replicated(nlls_ctx* ctx) { NLLS_API_BEGIN
    NEED_GRAD(); TRY(enqueue_solve_finish(ctx, TrialArgs{.replicate_xr = true})); drop(ctx->step.cached); return NLLS_OK;
    NLLS_API_END(ctx)
}
// this rank's share of a variable set: its own eliminated blocks' variables, on rank 0 also everything else; zeros elsewhere --
// the sum over ranks is the complete set (what a sharded optimisation hands back at the end)
int nlls_get_variables_owned(nlls_ctx* ctx, int32_t which, double* packed) { NLLS_API_BEGIN
    TRY(nlls_get_variables(ctx, which, packed));
    if (ctx->nranks == 1) return NLLS_OK;
    for (int64_t i = 0; i < ctx->info.nvar; ++i) {
        const uint64_t bi = ctx->blockindices[i];
        int owner = 0;
        if (bi > 0 && ctx->is_elim.size() >= bi && ctx->is_elim[bi - 1] && !ctx->owner_of_block.empty()) owner = ctx->owner_of_block[bi - 1];
        if (owner != ctx->rank) for (uint32_t q = ctx->var_off[i]; q < ctx->var_off[i + 1]; ++q) packed[q] = 0.0;
    }
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// optimizesingles!(problem, options, indices)  src/optimize.jl:60-76,183-205
int nlls_optimize_singles(nlls_ctx* ctx, int64_t nsel, const int64_t* varindices, const int64_t* cptr, const int32_t* cgroup, const int64_t* cindex,
                          const int32_t* cslot, int32_t iterator, int32_t maxiters, int32_t maxfails, double reldcost, double absdcost, double dstep, int64_t* iters_out) {
    NEED_READY();
    if (iterator < 0 || iterator > 3) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_optimize_singles: iterator must be 0 (Newton), 1 (Levenberg-Marquardt), 2 (dogleg) or 3 (gradient descent)");
    if (nsel < 0 || (nsel > 0 && (!varindices || !cptr))) return NLLS_ERR_INVALID_ARG;
    // Under nlls_set_shard (round 5; /root/reference/src/optimize.jl:60-76 is embarrassingly parallel per variable): every rank passes the SAME lists -- the caller's
    // variable and cost-block numbering -- and relaxes the variables whose cost blocks it owns (an eliminated variable's blocks all live on the rank that owns it:
    // build_structure); the results are gathered with the installed all-reduce, once.  A variable whose blocks are spread over ranks (a camera) is declined on every rank.
    const bool sharded = ctx->nranks > 1;
    if (sharded && (!ctx->reduce_fn || ctx->presharded)) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_optimize_singles under nlls_set_shard needs an installed all-reduce and a library-partitioned upload (not NLLS_FLAG_PRESHARDED)");
    if (nsel == 0) return NLLS_OK;
    const int64_t nc = cptr[nsel];
    if (cptr[0] != 0 || nc < 0 || (nc > 0 && (!cgroup || !cindex || !cslot))) return NLLS_ERR_INVALID_ARG;
    for (int64_t i = 0; i < nsel; ++i) {
        const int64_t v = varindices[i] - 1;
        if (v < 0 || v >= ctx->info.nvar || cptr[i + 1] < cptr[i]) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_optimize_singles: bad variable index or cost list");
        if (var_dof(ctx->var_kind[v], ctx->var_dim[v]) > (ctx->var_kind[v] == NLLS_VAR_DYNAMIC ? 6 : NLLS_SINGLES_MAX_DOF)) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_optimize_singles: variable with more than 12 degrees of freedom (NLLS_SINGLES_MAX_DOF; a dynamic-size one: 6)");
    }
    // this rank's share: the variables all of whose blocks are local, with the blocks' LOCAL indices -- in three runs, one per kernel: a variable of more than 6 dof, or of
    // at least singles_wave_min blocks, gets a wavefront (below that a wavefront has idle lanes in its only pass, while the thread kernel packs 64 variables into one)
    std::vector<int64_t> sel, cp(1, 0), pos; std::vector<uint32_t> cidx; std::vector<int32_t> cg, cs; double spread = 0.0; int64_t nrun[3] = {0, 0, 0};
    sel.reserve((size_t)nsel); cidx.reserve((size_t)nc); cg.reserve((size_t)nc); cs.reserve((size_t)nc);
    for (int run = 0; run < 3; ++run)
    for (int64_t i = 0; i < nsel; ++i) {
        const int dof = var_dof(ctx->var_kind[varindices[i] - 1], ctx->var_dim[varindices[i] - 1]);
        if (run != (dof > 6 ? 2 : std::max<int64_t>(cptr[i + 1] - cptr[i], 1) >= ctx->sw.singles_wave_min ? 1 : 0)) continue;      // (an empty list counts as one block: NLLS_SINGLES_WAVE_MIN=1 sends everything to the wavefront kernel)
        int64_t mine = 0; const size_t mark = cidx.size();
        for (int64_t e = cptr[i]; e < cptr[i + 1]; ++e) {
            if (cgroup[e] < 0 || cgroup[e] >= (int32_t)ctx->groups.size()) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_optimize_singles: bad cost group");
            const Group& G = ctx->groups[cgroup[e]];
            const int64_t nglob = G.local_of.empty() ? G.ncost : (int64_t)G.local_of.size();
            if (cindex[e] < 0 || cindex[e] >= nglob || cslot[e] < 0 || cslot[e] >= G.ndeps) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_optimize_singles: bad cost index or slot");
            if (G.adaptive && cslot[e] == 0) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_optimize_singles: the adaptive kernel variable cannot be optimised on its own");
            if (is_dyn_kind(G.res_kind)) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_optimize_singles: dynamic-size cost blocks are not handled by the per-variable kernel");
            const int64_t loc = G.local_of.empty() ? cindex[e] : (int64_t)G.local_of[(size_t)cindex[e]];
            if (loc >= 0) { ++mine; cidx.push_back((uint32_t)loc); cg.push_back(cgroup[e]); cs.push_back(cslot[e]); }
        }
        const int64_t all = cptr[i + 1] - cptr[i];
        // a variable without any block is relaxed (trivially) by rank 0
        if (mine == all && (all > 0 || ctx->rank == 0 || !sharded)) { sel.push_back(varindices[i] - 1); pos.push_back(i); cp.push_back((int64_t)cidx.size()); ++nrun[run]; }
        else { cidx.resize(mark); cg.resize(mark); cs.resize(mark); if (mine != 0) spread = 1.0; }
    }
    if (sharded) {          // a variable whose blocks are spread over ranks: declined everywhere (one small collective, so that no rank is left in the gather below)
        DevBuf<double> df; HIP_TRY(ctx, df.alloc(1)); HIP_TRY(ctx, hipMemcpyAsync(df.p, &spread, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        TRY(comm_reduce(ctx, df.p, 1, NLLS_REDUCE_MAX));
        HIP_TRY(ctx, hipMemcpyAsync(&spread, df.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream)); HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (spread != 0.0) return fail(ctx, NLLS_ERR_UNSUPPORTED, "nlls_optimize_singles under nlls_set_shard: a listed variable's cost blocks are spread over ranks (only variables whose blocks one rank owns -- the eliminated ones -- are relaxed in parallel)");
    }
    const int64_t nloc = (int64_t)sel.size();
    std::vector<unsigned char> gbuf(singles_group_size() * ctx->groups.size());
    for (size_t g = 0; g < ctx->groups.size(); ++g) singles_group_fill(gbuf.data() + g * singles_group_size(), ctx->groups[g]);
    DevBuf<int64_t> d_sel, d_cptr, d_iters, d_pos, d_all; DevBuf<int32_t> d_cgroup, d_cslot; DevBuf<uint32_t> d_cidx; DevBuf<unsigned char> d_groups;
    if (cidx.empty()) { cidx.push_back(0); cg.push_back(0); cs.push_back(0); }
    if (nloc > 0) { HIP_TRY(ctx, d_sel.upload(sel)); HIP_TRY(ctx, d_cptr.upload(cp)); HIP_TRY(ctx, d_cgroup.upload(cg)); HIP_TRY(ctx, d_cslot.upload(cs)); HIP_TRY(ctx, d_cidx.upload(cidx)); HIP_TRY(ctx, d_iters.alloc((size_t)nloc)); }
    HIP_TRY(ctx, d_groups.upload(gbuf));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    vars_written(ctx, NLLS_VARS_CURRENT, true);
    ctx->singles_thread = nrun[0]; ctx->singles_wave = nrun[1] + nrun[2];
    if (nloc > 0) TRY(enqueue_optimize_singles(ctx, nrun[0], nrun[1], nrun[2], d_sel.p, d_cptr.p, d_cgroup.p, d_cidx.p, d_cslot.p, d_groups.p, iterator, maxiters, maxfails, reldcost, absdcost, dstep, d_iters.p));
    if (!sharded) {
        std::vector<int64_t> hit((size_t)nsel);                                                                        // (unsharded: nloc == nsel, in the order of the runs)
        if (iters_out) HIP_TRY(ctx, hipMemcpyAsync(hit.data(), d_iters.p, sizeof(int64_t) * nsel, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (iters_out) for (int64_t i = 0; i < nsel; ++i) iters_out[pos[(size_t)i]] = hit[(size_t)i];
        return NLLS_OK;
    }
    // the gather: [storage of the variables this rank relaxed, zero elsewhere | their iteration counts at the caller's positions] summed over ranks; then every listed
    // variable's storage is taken from the sum -- exact: each entry has one non-zero contribution
    const size_t nst = (size_t)ctx->info.var_storage; DevBuf<double> gb; HIP_TRY(ctx, gb.alloc(nst + (size_t)nsel));
    HIP_TRY(ctx, hipMemsetAsync(gb.p, 0, sizeof(double) * (nst + (size_t)nsel), ctx->stream));
    double* cur = vars_ptr(ctx, NLLS_VARS_CURRENT);
    if (nloc > 0) { HIP_TRY(ctx, d_pos.upload(pos)); TRY(enqueue_copy_var_storage(ctx, d_sel.p, nloc, cur, gb.p)); TRY(enqueue_iters_to_double(ctx, d_iters.p, d_pos.p, nloc, gb.p + nst)); }
    TRY(comm_reduce(ctx, gb.p, (int64_t)(nst + (size_t)nsel), NLLS_REDUCE_SUM));
    { std::vector<int64_t> all((size_t)nsel); for (int64_t i = 0; i < nsel; ++i) all[(size_t)i] = varindices[i] - 1; HIP_TRY(ctx, d_all.upload(all)); }
    TRY(enqueue_copy_var_storage(ctx, d_all.p, nsel, gb.p, cur));
    std::vector<double> hit((size_t)nsel);
    HIP_TRY(ctx, hipMemcpyAsync(hit.data(), gb.p + nst, sizeof(double) * (size_t)nsel, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (iters_out) for (int64_t i = 0; i < nsel; ++i) iters_out[i] = (int64_t)hit[(size_t)i];
    return NLLS_OK;
}
int nlls_get_time_buckets(nlls_ctx* ctx, int64_t* out, int32_t n) { NLLS_API_BEGIN
    if (!ctx || !out || n < 1) return NLLS_ERR_INVALID_ARG;
    const int64_t v[4] = {ctx->tb_grad_ns, ctx->tb_cost_ns, ctx->tb_solver_ns, ctx->tb_trials};
    for (int i = 0; i < n && i < 4; ++i) out[i] = v[i];
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_get_phase_times(nlls_ctx* ctx, double* out, int32_t n) { NLLS_API_BEGIN
    if (!ctx || !out || n < 1) return NLLS_ERR_INVALID_ARG;
    if (take(ctx->upd_pending) && ctx->phase_ev.size() >= 10) { float ms = 0.f; (void)hipSetDevice(ctx->device);
        if (hipEventSynchronize(ctx->phase_ev[9]) == hipSuccess && hipEventElapsedTime(&ms, ctx->phase_ev[8], ctx->phase_ev[9]) == hipSuccess) ctx->upd_ms = ms; else (void)hipGetLastError(); }
    if (take(ctx->lin_pending) && ctx->phase_ev.size() >= 12) { float ms = 0.f; (void)hipSetDevice(ctx->device);
        if (hipEventSynchronize(ctx->phase_ev[11]) == hipSuccess && hipEventElapsedTime(&ms, ctx->phase_ev[10], ctx->phase_ev[11]) == hipSuccess) ctx->lin_ms = ms; else (void)hipGetLastError(); }
    if (take(ctx->app_pending) && ctx->phase_ev.size() >= 14) { float ms = 0.f; (void)hipSetDevice(ctx->device);
        if (hipEventSynchronize(ctx->phase_ev[13]) == hipSuccess && hipEventElapsedTime(&ms, ctx->phase_ev[12], ctx->phase_ev[13]) == hipSuccess) ctx->app_ms = ms; else (void)hipGetLastError(); }
    if (take(ctx->pcg_pending) && ctx->phase_ev.size() >= 16) { float ms = 0.f; (void)hipSetDevice(ctx->device);
        if (hipEventSynchronize(ctx->phase_ev[15]) == hipSuccess && hipEventElapsedTime(&ms, ctx->phase_ev[14], ctx->phase_ev[15]) == hipSuccess) ctx->pcg_ms = ms; else (void)hipGetLastError(); }
    const double v[15] = {ctx->phase_ms[0], ctx->phase_ms[1], ctx->phase_ms[2], ctx->phase_ms[3], ctx->phase_ms[4], ctx->phase_ms[5], (double)ctx->phase_trials, (double)ctx->phase_sweeps, ctx->upd_ms, (double)ctx->upd_copies,
                          ctx->lin_ms, ctx->lin_bytes, ctx->app_ms, ctx->app_bytes, ctx->pcg_ms};
    for (int i = 0; i < n && i < 15; ++i) out[i] = v[i];
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_set_option(nlls_ctx* ctx, int32_t option, int64_t value) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    switch (option) {
    case NLLS_OPT_MATERIALIZE: ctx->sw.mf_on = value == 0; return NLLS_OK;          // (takes effect with the next nlls_lm_trial / nlls_sweep_gradhess; what A and b hold is tracked either way)
    case NLLS_OPT_LOOKAHEAD:   ctx->sw.spec_on = value != 0; return NLLS_OK;
    case NLLS_OPT_PHASE_EVENTS:
        ctx->phase_on = value != 0; (void)hipSetDevice(ctx->device);
        if (ctx->phase_on && ctx->phase_ev.empty()) { ctx->phase_ev.resize(16); for (auto& e : ctx->phase_ev) if (hipEventCreate(&e) != hipSuccess) return NLLS_ERR_HIP; }
        if (ctx->phase_on) { for (double& v : ctx->phase_ms) v = 0.0; ctx->phase_trials = ctx->phase_sweeps = 0; }
        return NLLS_OK;
    case NLLS_OPT_APPLY_SCRATCH:  if (value < 0) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_option: NLLS_OPT_APPLY_SCRATCH takes bytes"); ctx->app_scratch_cap = value; return NLLS_OK;
    case NLLS_OPT_APPLY_WAVE_MIN: ctx->app_wave_min = std::max<int64_t>(value, 1); return NLLS_OK;      // (the rows are classed again by the next product)
    case NLLS_OPT_PCG_ROUND:    if (value < 1) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_option: NLLS_OPT_PCG_ROUND takes iterations >= 1"); ctx->pcg_round = value; return NLLS_OK;
    case NLLS_OPT_PCG_GRID_MAX: if (value < 1) return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_option: NLLS_OPT_PCG_GRID_MAX takes workgroups >= 1"); ctx->pcg_grid_max = value; return NLLS_OK;
    }
    return fail(ctx, NLLS_ERR_INVALID_ARG, "nlls_set_option: unknown option");
    NLLS_API_END(ctx)
}
int nlls_get_solve_stats(nlls_ctx* ctx, int64_t* out, int32_t n) { NLLS_API_BEGIN
    NEED_READY(); if (!out || n < 1) return NLLS_ERR_INVALID_ARG;
    int32_t status[16] = {0};
    HIP_TRY(ctx, hipMemcpyAsync(status, ctx->d_status.p, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int64_t chain_form = 0, chain_window = 0; chain_form_stats(ctx, chain_form, chain_window);
    const int64_t vals[56] = {status[0], (int64_t)status[2] << 10, (int64_t)status[3] << 10, ctx->solve_mode, ctx->nelim_groups, ctx->bw,
                              ctx->bcr.ready ? ctx->bcr.mfma_issued : 0, ctx->bcr.ready ? ctx->bcr.launches : 0, ctx->bcr.ready ? (int64_t)ctx->bcr.levels.size() : 0, ctx->n_band,
                              status[4] /* pivots the floor of the last undamped band solve dropped */, ctx->n_stage0, ctx->n_lazy_trials, ctx->red_reordered, ctx->bw_caller, ctx->dense_window ? 1 : 0,
                              ctx->tsp.ready ? ctx->tsp.nt : 0, ctx->tsp.ready ? (int64_t)ctx->tsp.levels.size() : 0, ctx->tsp.ready ? ctx->tsp.nslots : 0, ctx->tsp.ready ? ctx->tsp.launches : 0, ctx->tsp.ready ? ctx->tsp.products : 0,
                              ctx->ahead.hits, ctx->ahead.misses /* look-ahead sweeps used / thrown away */,
                              ctx->mf_trials, ctx->mf_reduced_sweeps, ctx->full_sweeps /* matrix-free LM trials, sweeps of the reduced rows only, full accumulate sweeps since the upload */,
                              ctx->bcr.ready ? 16 * ctx->bcr.NT : 0 /* unknowns per block of the block cyclic reduction */,
                              ctx->singles_wave, ctx->singles_thread /* variables the last nlls_optimize_singles call relaxed one per wavefront / one per thread */,
                              // [29..36] the elimination as the upload classed it: fast supernodes of at most 60 / 61..63 / 64..70 neighbour unknowns, generic (LDS-staged) supernodes with / without
                              // pair accumulators, neighbour blocks read transposed (stored in the neighbour's row) / in all, the slab + gather assembly of the materialised elimination in use
                              ctx->n_fast_n60, ctx->n_fast_narrow - ctx->n_fast_n60, ctx->n_fast_groups - ctx->n_fast_narrow, ctx->n_slow_acc, ctx->n_slow_groups - ctx->n_slow_acc,
                              ctx->n_elim_nbrs_trans, ctx->n_elim_nbrs, ctx->elim_slab ? 1 : 0,
                              // [37..42] the accumulate sweep, summed over groups (and slots): light tiles, heavy tiles with an LDS image, TILE_DIRECT tiles, TILE_PARTIAL tiles (light or heavy),
                              // folded groups, groups whose last full sweep was one fused launch
                              ctx->n_tiles_light, ctx->n_tiles_image, ctx->n_tiles_direct, ctx->n_tiles_partial, ctx->n_fold_groups, ctx->sweep_fused_groups,
                              // [43..46] nlls_eval_jacobians / nlls_eval_gradhess: doubles of LDS a wavefront stages records in; lanes per staged sub-batch of the last call's J / g / H (0: stored directly)
                              lin_wave_slab(), ctx->lin_batch[0], ctx->lin_batch[1], ctx->lin_batch[2],
                              // [47..50] the last matrix-free product (nlls_apply.hip): rows gathered one lane per unknown / a wavefront each, chunks of vectors, doubles of record scratch
                              ctx->app_short, ctx->app_long, ctx->app_chunks, ctx->app_scratch,
                              // [51], [52] the band solver's form where the chain kernels solve the band (0: they do not; 1 register window, 2 blocked one-sided, 3 blocked twisted) and,
                              // for form 1, the window 1000 SEG + 10 NSLOT + CH / 8
                              chain_form, chain_window,
                              // [53..55] the last nlls_solve_pcg: iterations made, status, synchronisations
                              ctx->pcg_iters, ctx->pcg_status, ctx->pcg_rounds};
    for (int i = 0; i < n && i < 56; ++i) out[i] = vals[i];
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_set_step(nlls_ctx* ctx, const double* x) { NLLS_API_BEGIN
    NEED_READY(); if (!x) return NLLS_ERR_INVALID_ARG;
    step_replaced(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->x.p, x, sizeof(double) * ctx->info.ndof, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_get_step(nlls_ctx* ctx, double* x_out) { NLLS_API_BEGIN
    NEED_READY(); if (!x_out) return NLLS_ERR_INVALID_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(x_out, ctx->x.p, sizeof(double) * ctx->info.ndof, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_step_maxabs(nlls_ctx* ctx, double* out) { NLLS_API_BEGIN
    NEED_READY(); if (ctx->step.cached) { if (out) *out = ctx->step.maxabs; return NLLS_OK; }
    TRY(enqueue_step_stats(ctx)); TRY(fetch_scalars(ctx, 1, 2));
    if (out) *out = ctx->h_scalars[1]; return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_step_norm(nlls_ctx* ctx, double* out) { NLLS_API_BEGIN
    NEED_READY(); if (ctx->step.cached) { if (out) *out = std::sqrt(ctx->step.sumsq); return NLLS_OK; }
    TRY(enqueue_step_stats(ctx)); TRY(fetch_scalars(ctx, 1, 2));
    if (out) *out = std::sqrt(ctx->h_scalars[2]); return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_quadform(nlls_ctx* ctx, double* xHx_out, double* gx_out) { NLLS_API_BEGIN
    NEED_GRAD_LAZY();
    if (ctx->step.cached) { if (xHx_out) *xHx_out = ctx->step.xAx + ctx->lambda * ctx->step.xx; if (gx_out) *gx_out = ctx->step.gx; return NLLS_OK; }   // damping may have changed since
    TRY(ensure_grad(ctx, 2)); TRY(ensure_reduced_summed(ctx));
    TRY(enqueue_quadform(ctx, ctx->x.p, 4)); TRY(comm_reduce(ctx, ctx->scalars.p + 4, 2, NLLS_REDUCE_SUM)); TRY(fetch_scalars(ctx, 4, 2));
    if (xHx_out) *xHx_out = ctx->h_scalars[4]; if (gx_out) *gx_out = ctx->h_scalars[5];
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_retract(nlls_ctx* ctx, int32_t to, int32_t from) { NLLS_API_BEGIN
    NEED_READY(); if (!valid_set(to) || !valid_set(from) || to == from) return NLLS_ERR_INVALID_ARG;
    TRY(vars_written(ctx, to));
    return enqueue_retract(ctx, to, from);
    NLLS_API_END(ctx)
}

// ---- multi-GPU: local phases + reduce buffers.  Under nlls_set_shard(rank, nranks > 1):
//   nlls_sweep_cost / nlls_quadform / nlls_max_abs_diag / nlls_grad_* return this rank's PARTIAL values (the caller
//   sums, or takes the max of, them over ranks); the *_local / *_finish pairs bracket the buffer reductions.
int nlls_sweep_gradhess_local(nlls_ctx* ctx) { NLLS_API_BEGIN
    NEED_READY(); drop_lookahead(ctx, true); TRY(enqueue_sweep_gradhess(ctx));
    new_linearisation(ctx);                          // (the caller sums the reduce buffer)
    if (ctx->nranks > 1) TRY(enqueue_pack_reduce0(ctx));
    return NLLS_OK;                                  // enqueue only: the reduce buffer is complete in stream order
    NLLS_API_END(ctx)
}
int nlls_sweep_gradhess_finish(nlls_ctx* ctx, double* cost_out) { NLLS_API_BEGIN
    NEED_GRAD();
    if (ctx->nranks > 1) TRY(enqueue_unpack_reduce0(ctx));
    if (!cost_out) return NLLS_OK;                   // cost not wanted (src/optimize.jl:169 discards it): no synchronisation
    TRY(fetch_scalars(ctx, 0, 1)); *cost_out = ctx->h_scalars[0]; return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_sweep_cost_local(nlls_ctx* ctx, int32_t which) { NLLS_API_BEGIN NEED_READY(); if (!valid_set(which)) return NLLS_ERR_INVALID_ARG; return enqueue_sweep_cost(ctx, which); NLLS_API_END(ctx) }
int nlls_sweep_cost_finish(nlls_ctx* ctx, double* cost_out) { NLLS_API_BEGIN NEED_READY(); TRY(fetch_scalars(ctx, 0, 1)); if (cost_out) *cost_out = ctx->h_scalars[0]; return NLLS_OK; NLLS_API_END(ctx) }
int nlls_solve_local(nlls_ctx* ctx) { NLLS_API_BEGIN
    NEED_GRAD(); TRY(enqueue_solve_local(ctx));
    return NLLS_OK;                                  // enqueue only, as above
    NLLS_API_END(ctx)
}
int nlls_solve_finish(nlls_ctx* ctx, double* x_out) { NLLS_API_BEGIN
    NEED_GRAD(); TRY(enqueue_solve_finish(ctx));
    int32_t status[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(status, ctx->d_status.p, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
    if (x_out) HIP_TRY(ctx, hipMemcpyAsync(x_out, ctx->x.p, sizeof(double) * ctx->info.ndof, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (status[0] != 0) return status_error(ctx, status[0], "factorisation met a zero pivot");
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_solve_finish_async(nlls_ctx* ctx) { NLLS_API_BEGIN           // enqueue only: the status comes home with nlls_trial_local's scalars
    NEED_GRAD(); TRY(enqueue_solve_finish(ctx)); drop(ctx->step.cached); return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_get_reduce_buffer(nlls_ctx* ctx, int32_t stage, void** dev_ptr, int64_t* count) { NLLS_API_BEGIN
    NEED_READY(); if (!dev_ptr || !count) return NLLS_ERR_INVALID_ARG;
    if (stage == 0) { *dev_ptr = ctx->redbuf.p; *count = ctx->redbuf_len; return NLLS_OK; }                                   // after sweep_gradhess_local
    if (stage == 1) { *dev_ptr = ctx->S.p; *count = (int64_t)ctx->s_elems + ctx->nred; return NLLS_OK; }                      // after solve_local: [S | s]
    if (stage == 2) { *dev_ptr = ctx->x.p; *count = ctx->info.ndof; return NLLS_OK; }                                         // after solve_finish: x
    // after nlls_trial_local(out = NULL): the trial's scalars, to be GATHERED (not summed) -- [0] cost, [8] x'Hx, [5] g'x (partial sums),
    // [1] max|x|, [9] |x|^2 over this rank's share of the step, [10] factorisation status
    if (stage == 3) { *dev_ptr = ctx->scalars.p; *count = 11; return NLLS_OK; }
    return fail(ctx, NLLS_ERR_INVALID_ARG, "unknown reduce stage");
    NLLS_API_END(ctx)
}
int nlls_get_step_shard(nlls_ctx* ctx, void** dev_ptr_x, int64_t* reduced_count, int64_t* own_offset, int64_t* own_count) { NLLS_API_BEGIN
    NEED_READY();
    if (dev_ptr_x) *dev_ptr_x = ctx->x.p; if (reduced_count) *reduced_count = ctx->nred;
    if (own_offset) *own_offset = 0; if (own_count) *own_count = ctx->info.ndof;
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_get_grad_owned(nlls_ctx* ctx, double* b_out) { NLLS_API_BEGIN
    TRY(nlls_get_grad(ctx, b_out));
    if (ctx->nranks > 1) {
        std::vector<double> mask((size_t)ctx->info.ndof);
        HIP_TRY(ctx, hipMemcpy(mask.data(), ctx->d_dof_mask.p, sizeof(double) * mask.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < mask.size(); ++i) if (mask[i] == 0.0) b_out[i] = 0.0;
    }
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_get_shard_info(nlls_ctx* ctx, int64_t* out, int32_t n) { NLLS_API_BEGIN
    NEED_READY(); if (!out || n < 1) return NLLS_ERR_INVALID_ARG;
    const int64_t vals[6] = {ctx->rank, ctx->nranks, ctx->local_ncost, ctx->local_nnz_data, ctx->local_ndof, ctx->replicated ? ctx->shard_nranks : 0};
    for (int i = 0; i < n && i < 6; ++i) out[i] = vals[i];
    return NLLS_OK;
    NLLS_API_END(ctx)
}

// ---- timing helpers: HIP events on the context's stream around `reps` back-to-back enqueues -------------
static int time_loop(nlls_ctx* ctx, int reps, float* ms_avg, int (*fn)(nlls_ctx*)) {
    if (reps < 1 || !ms_avg) return NLLS_ERR_INVALID_ARG;
    hipEvent_t e0, e1; HIP_TRY(ctx, hipEventCreate(&e0)); HIP_TRY(ctx, hipEventCreate(&e1));
    TRY(fn(ctx));   // warm-up
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < reps; ++i) TRY(fn(ctx));
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    float ms = 0; HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    *ms_avg = ms / reps;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return NLLS_OK;
}

// (the timed sweeps leave A and b the linearisation at CURRENT, outside the look-ahead protocol and with the damping kept)
static int time_sweeps(nlls_ctx* ctx, int reps, float* ms_avg, int (*fn)(nlls_ctx*)) { drop_lookahead(ctx, false); int rc = time_loop(ctx, reps, ms_avg, fn); new_linearisation(ctx, true, false); return rc; }
int nlls_time_sweep_gradhess(nlls_ctx* ctx, int32_t reps, float* ms_avg) { NLLS_API_BEGIN
    NEED_READY(); return time_sweeps(ctx, reps, ms_avg, [](nlls_ctx* c) { return enqueue_sweep_gradhess(c); }); NLLS_API_END(ctx) }
int nlls_time_sweep_accumulate(nlls_ctx* ctx, int32_t reps, float* ms_avg) { NLLS_API_BEGIN
    NEED_READY(); return time_sweeps(ctx, reps, ms_avg, [](nlls_ctx* c) { return enqueue_sweep_gradhess(c, false); }); NLLS_API_END(ctx) }
int nlls_time_sweep_cost(nlls_ctx* ctx, int32_t reps, float* ms_avg) { NLLS_API_BEGIN
    NEED_READY(); return time_loop(ctx, reps, ms_avg, [](nlls_ctx* c) { return enqueue_sweep_cost(c, NLLS_VARS_CURRENT); });
    NLLS_API_END(ctx)
}
int nlls_time_solve(nlls_ctx* ctx, int32_t reps, float* ms_avg) { NLLS_API_BEGIN
    NEED_GRAD(); return time_loop(ctx, reps, ms_avg, [](nlls_ctx* c) { return enqueue_solve(c); });
    NLLS_API_END(ctx)
}
int nlls_get_memory_info(nlls_ctx* ctx, int64_t* out, int32_t n) { NLLS_API_BEGIN
    NEED_READY(); if (!out || n < 4) return NLLS_ERR_INVALID_ARG;
    out[0] = ctx->hot_bytes; out[1] = (int64_t)ctx->arena.n; out[2] = (int64_t)sizeof(double) * ctx->info.nnz_data; out[3] = (int64_t)sizeof(double) * ((int64_t)ctx->s_elems + ctx->nred);
    if (n >= 5) out[4] = (int64_t)sizeof(double) * ((ctx->solve_mode == SOLVE_TSPARSE ? ctx->tsp.nslots_assembled * (int64_t)TSP_TE : (int64_t)ctx->s_elems) + ctx->nred);   // what a sharded trial sums over ranks
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_check_analytic(nlls_ctx* ctx, double* out, int32_t n) { NLLS_API_BEGIN
    NEED_READY(); if (!out || n < 7) return NLLS_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    int64_t nb = 0; TRY(enqueue_check_analytic(ctx, nullptr, &nb));
    for (int q = 0; q < 7; ++q) out[q] = 0.0;
    if (nb == 0) return NLLS_OK;
    nlls::DevBuf<double> d; HIP_TRY(ctx, d.alloc((size_t)nb * 8));
    TRY(enqueue_check_analytic(ctx, d.p, nullptr));
    std::vector<double> h((size_t)nb * 8);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), d.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream)); HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < nb; ++b) for (int q = 0; q < 7; ++q) { const double v = h[(size_t)b * 8 + q]; if (!(v <= out[q])) out[q] = v; }   // (a NaN difference comes through)
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// robustify / robustifydcost, src/robust.jl:11-14,26-31,47-55,71-77 (user kernels: their robustify and autorobustifydcost, src/autodiff.jl:163)
int nlls_robustify(nlls_ctx* ctx, int32_t robust_kind, const double params[4], int64_t n, const double* cost, double* out) { NLLS_API_BEGIN
    if (!ctx || !params || n < 0 || (n > 0 && (!cost || !out)) || n > ((int64_t)1 << 32)) return NLLS_ERR_INVALID_ARG;
    if (robust_nparams(robust_kind & 0xF) < 0 || (robust_kind & ~0x1F)) return fail(ctx, NLLS_ERR_UNSUPPORTED, "unregistered robust kernel");
    if (n == 0) return NLLS_OK;
    (void)hipSetDevice(ctx->device);
    RobustSpec rk{}; rk.kind = robust_kind; rk.p0 = params[0]; rk.p1 = params[1]; rk.p2 = params[2];
    nlls::DevBuf<double> d; HIP_TRY(ctx, d.alloc((size_t)n * 5));
    HIP_TRY(ctx, hipMemcpyAsync(d.p, cost, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    TRY(enqueue_robustify(ctx, rk, n, d.p, d.p + n));
    HIP_TRY(ctx, hipMemcpyAsync(out, d.p + n, sizeof(double) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream)); HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_flush_cache(nlls_ctx* ctx, int64_t bytes) { NLLS_API_BEGIN
    if (!ctx || bytes <= 0 || bytes > ((int64_t)8 << 30)) return NLLS_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    const size_t half = ((size_t)bytes / 2 + 255) & ~(size_t)255;
    if (ctx->flushbuf.n < 2 * half) { HIP_TRY(ctx, ctx->flushbuf.alloc(2 * half)); HIP_TRY(ctx, hipMemsetAsync(ctx->flushbuf.p, 1, 2 * half, ctx->stream)); }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->flushbuf.p + half, ctx->flushbuf.p, half, hipMemcpyDeviceToDevice, ctx->stream));
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_profile_sweep(nlls_ctx* ctx, int32_t on, float* ms_avg, float* ms_min, float* ms_max, int64_t* nsamples) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    if (ms_avg || ms_min || ms_max || nsamples) {            // read what has been recorded so far (synchronises the stream)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const int64_t cap = (int64_t)ctx->prof_ev.size() / 2, n = std::min(ctx->prof_count, cap);
        double sum = 0; float mn = 1e30f, mx = 0.f;
        for (int64_t i = 0; i < n; ++i) { float ms = 0.f; if (hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]) != hipSuccess) continue; sum += ms; mn = std::min(mn, ms); mx = std::max(mx, ms); }
        // where the fused accumulate kernel stamped itself (first workgroup start .. last workgroup end), that span is the figure:
        // it is what a kernel trace reports for the launch; the event pairs also hold the dispatch latency in front of it
        const int64_t nk = std::min<int64_t>(ctx->prof_kcount, PROF_SLOTS);
        if (nk > 0 && ctx->prof_clk.p) {
            std::vector<unsigned long long> h(2 * (size_t)PROF_MAXWG);
            sum = 0; mn = 1e30f; mx = 0.f; int64_t ok = 0;
            int khz = 100000; (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device); if (khz <= 0) khz = 100000;
            const double ms_per_tick = 1.0 / (double)khz;
            for (int64_t i = 0; i < nk; ++i) {
                const unsigned nwg = ctx->prof_nwg[i]; if (!nwg) continue;
                HIP_TRY(ctx, hipMemcpy(h.data(), ctx->prof_clk.p + (size_t)i * 2 * PROF_MAXWG, sizeof(unsigned long long) * 2 * (size_t)nwg, hipMemcpyDeviceToHost));
                unsigned long long t0 = ~0ull, t1 = 0; for (unsigned w = 0; w < nwg; ++w) { t0 = std::min(t0, h[w]); t1 = std::max(t1, h[nwg + w]); }
                if (t1 <= t0) continue;
                const float ms = (float)((double)(t1 - t0) * ms_per_tick); sum += ms; mn = std::min(mn, ms); mx = std::max(mx, ms); ++ok;
            }
            if (ms_avg) *ms_avg = ok ? (float)(sum / ok) : 0.f; if (ms_min) *ms_min = ok ? mn : 0.f; if (ms_max) *ms_max = mx; if (nsamples) *nsamples = ok;
        } else {
            if (ms_avg) *ms_avg = n ? (float)(sum / n) : 0.f; if (ms_min) *ms_min = n ? mn : 0.f; if (ms_max) *ms_max = mx; if (nsamples) *nsamples = n;
        }
    }
    if (on && !ctx->prof_clk.p) { if (ctx->prof_clk.alloc((size_t)PROF_SLOTS * 2 * PROF_MAXWG) != hipSuccess) return NLLS_ERR_HIP; }
    if (on) ctx->prof_kcount = 0;
    if (on && ctx->prof_ev.empty()) { ctx->prof_ev.resize(128); for (auto& e : ctx->prof_ev) if (hipEventCreate(&e) != hipSuccess) return NLLS_ERR_HIP; }
    ctx->prof_sweep = on != 0; if (on) ctx->prof_count = 0;
    return NLLS_OK;
    NLLS_API_END(ctx)
}
// the event pairs alone: begin .. end of the accumulate dispatch(es) as the command processor stamped them -- what rocprofv3 --kernel-trace reports per dispatch
int nlls_profile_sweep_dispatch(nlls_ctx* ctx, float* ms_avg, float* ms_min, float* ms_max, int64_t* nsamples) { NLLS_API_BEGIN
    if (!ctx) return NLLS_ERR_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t cap = (int64_t)ctx->prof_ev.size() / 2, n = std::min(ctx->prof_count, cap);
    double sum = 0; float mn = 1e30f, mx = 0.f; int64_t ok = 0;
    for (int64_t i = 0; i < n; ++i) { float ms = 0.f; if (hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]) != hipSuccess) { (void)hipGetLastError(); continue; } sum += ms; mn = std::min(mn, ms); mx = std::max(mx, ms); ++ok; }
    if (ms_avg) *ms_avg = ok ? (float)(sum / ok) : 0.f; if (ms_min) *ms_min = ok ? mn : 0.f; if (ms_max) *ms_max = mx; if (nsamples) *nsamples = ok;
    return NLLS_OK;
    NLLS_API_END(ctx)
}
int nlls_time_reduced_solve(nlls_ctx* ctx, int32_t reps, float* ms_avg) { NLLS_API_BEGIN
    NEED_GRAD();
    if (ctx->nred == 0 || ctx->elim_slab) { if (ms_avg) *ms_avg = 0.f; return NLLS_OK; }   // (slab + gather assembly: the tiles are consumed in place)
    if (ctx->solve_mode == SOLVE_BAND && ctx->bcr.ready) {
        // block cyclic reduction copies [S | s] into its own tiles: assemble once, then time the factorisation + backward pass alone
        TRY(enqueue_solve_local(ctx));
        const int rc = time_loop(ctx, reps, ms_avg, [](nlls_ctx* c) { return enqueue_reduced_solve(c); });
        drop(ctx->zero.S);
        return rc;
    }
    // the dense, one-wave and chain solvers factor S IN PLACE: every repetition assembles it again, and the assembly alone is timed and subtracted
    float ms_both = 0.f, ms_asm = 0.f;
    int rc = time_loop(ctx, reps, &ms_both, [](nlls_ctx* c) { drop(c->zero.S); int r = enqueue_solve_local(c); return r != NLLS_OK ? r : enqueue_reduced_solve(c); });
    if (rc == NLLS_OK) rc = time_loop(ctx, reps, &ms_asm, [](nlls_ctx* c) { drop(c->zero.S); return enqueue_solve_local(c); });
    drop(ctx->zero.S);
    if (ms_avg) *ms_avg = ms_both > ms_asm ? ms_both - ms_asm : 0.f;
    return rc;
    NLLS_API_END(ctx)
}

}  // extern "C"
