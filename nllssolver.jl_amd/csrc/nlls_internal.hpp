// nlls_internal.hpp -- declarations shared by the translation units of libnlls_amd.so
#pragma once

#include <cmath>
#include <exception>
#include <new>

#include "nlls_ctx.hpp"

#define NLLS_FOR_EACH_RES(X) \
    X(NLLS_RES_BA_AFFINE) X(NLLS_RES_ROSENBROCK_A) X(NLLS_RES_ROSENBROCK_B) X(NLLS_RES_ROSENBROCK_2D) \
    X(NLLS_RES_CURVE_EXP4) X(NLLS_RES_ADAPTIVE_MEAN) X(NLLS_RES_BA_SO3) X(NLLS_RES_BA_SO3_ADAPTIVE) X(NLLS_RES_LINEAR3) X(NLLS_COST_LINEAR3) X(NLLS_RES_SCALE_MIX) NLLS_USER_RES(X)
#include "nlls_launch.hpp"

// Every extern "C" entry point runs between these two (nothing may throw or longjmp across the ccall boundary): a C++ exception -- std::bad_alloc of a host-side
// work vector, above all -- becomes NLLS_ERR_HIP with the message in nlls_last_error.
#define NLLS_API_BEGIN try {
#define NLLS_API_END(C) } catch (const std::bad_alloc&) { return nlls::api_exception(C, "out of host memory (std::bad_alloc)"); } \
    catch (const std::exception& e_) { return nlls::api_exception(C, e_.what()); } catch (...) { return nlls::api_exception(C, "unknown C++ exception"); }

namespace nlls {

inline int api_exception(nlls_ctx* c, const char* what) { if (c) { try { c->err = std::string("host exception: ") + what; } catch (...) {} } return NLLS_ERR_HIP; }

struct ResDesc { int ndeps, nres, ndata, adaptive; int sk[MAX_SLOTS], sd[MAX_SLOTS]; };
bool res_desc(int kind, ResDesc& d);
inline bool is_dyn_kind(int kind) { return kind >= NLLS_RES_DYN_LINEAR && kind <= NLLS_COST_DYN_LINEAR; }

int build_structure(nlls_ctx* c, int64_t nvar, const int32_t* var_kind, const int32_t* var_dim, const uint64_t* bi,
                    int32_t ngroups, const nlls_cost_group* groups, int32_t flags);
int select_elimination(nlls_ctx* c, int32_t flags);
int build_schur(nlls_ctx* c, int32_t flags);
std::vector<int32_t> rcm_order(const std::vector<std::vector<int32_t>>& adj);   // reverse Cuthill-McKee: perm[new position] = node (nlls_structure.cpp)

// One LM trial's solve and tail (default: a plain solve).  to / from: it retracts vars[from] + x into vars[to]; mf: matrix-free; replicate_xr: every rank writes the step's
// reduced part; zero_for_lookahead: the finishing launch zero-fills the rows of the look-ahead sweep behind it; defer_fin: matrix-free, the finishing workgroup rides in that
// sweep's launch; mirror: the pinned host mirror as the device sees it, where the tail publishes scalars and stamps -- set it by name where the host waits on them
struct TrialArgs { int to = -1, from = -1; bool mf = false, replicate_xr = false, zero_for_lookahead = false, defer_fin = false; double* mirror = nullptr;
                   double* stamps() const { return mirror ? mirror + 40 : nullptr; } };

// sweeps (nlls_sweep.hip): enqueue on c->stream; cost lands in c->scalars[0]
struct PostSolveArgs;
int enqueue_sweep_cost(nlls_ctx* c, int which, int64_t pofs = 0, int64_t* count = nullptr, const PostSolveArgs* post = nullptr, bool* post_taken = nullptr);   // post: the step-statistics roles of an LM trial ride in the first launch (nlls_post.hpp)
// (nlls_cost.hip) cost-only blocks and the final reduction of the cost partials, shared with the gradient sweep
int enqueue_fixedcost(nlls_ctx* c, const Group& G, const double* vars, int64_t& pbase);
int enqueue_dyn_gradhess(nlls_ctx* c, const Group& G, const double* vars, int64_t& pbase);   // dynamic-size residual blocks (dense system): accumulate
int enqueue_reduce_partials(nlls_ctx* c, int64_t n);
int enqueue_check_analytic(nlls_ctx* c, double* d_out, int64_t* nblocks_out);   // closed-form block maths against the dual-number statement (nlls_check_analytic)
int enqueue_robustify(nlls_ctx* c, const RobustSpec& rk, int64_t n, const double* d_cost, double* d_out);   // out[4 i ..] = robustify, rho, rho', rho'' at cost[i] (nlls_robustify)
int enqueue_sweep_gradhess(nlls_ctx* c, bool want_cost = true, int which = NLLS_VARS_CURRENT, int mode = 0);   // mode 1: the reduced rows only (the matrix-free trial's gradient sweep: nlls::Linearisation::level 1)   // which: the variable set to linearise at (the look-ahead sweep of an LM trial: NLLS_VARS_NEXT)
// vector helpers (nlls_sweep.hip)
int enqueue_retract(nlls_ctx* c, int to, int from);
int enqueue_step_stats(nlls_ctx* c);          // scalars[1] = max|x|, scalars[2] = x'x
int enqueue_max_abs_diag(nlls_ctx* c);        // scalars[3]
// optimizesingles! (nlls_cost.hip): all arrays on the device; d_groups = singles_group_size() bytes per cost group.  The variables in three runs: one per thread, then
// one per wavefront of at most 6 dof and of at most NLLS_SINGLES_MAX_DOF
int enqueue_optimize_singles(nlls_ctx* c, int64_t nthread, int64_t nwave6, int64_t nwave12, const int64_t* d_selvar, const int64_t* d_cptr, const int32_t* d_cgroup, const uint32_t* d_cidx,
                             const int32_t* d_cslot, const void* d_groups, int iterator, int maxiters, int maxfails, double reldcost, double absdcost, double dstep, int64_t* d_iters);
int enqueue_copy_var_storage(nlls_ctx* c, const int64_t* d_sel, int64_t nsel, const double* src, double* dst);      // the listed variables' storage, src -> dst (same layout)
int enqueue_iters_to_double(nlls_ctx* c, const int64_t* d_it, const int64_t* d_pos, int64_t n, double* d_out);
// per-block values and the adaptive kernel's EM step (nlls_eval.hip): device output pointers (null: not wanted); the EM call's state is left in c->em_state
int eval_nres(const Group& G);                 // residuals per block of the group (dynamic kinds: the run-time n)
int enqueue_eval_blocks(nlls_ctx* c, const Group& G, int which, double* d_r, double* d_sq, double* d_rho, double* d_w);
int enqueue_adaptive_em(nlls_ctx* c, int which, uint32_t kvoff, int maxiters);
// per-block linearisation (nlls_linearize.hip): n selected blocks of a group (d_index: their 1-based blocks on the device, null: the first n); device output pointers (null: not wanted)
struct LinSizes { int m, nj, p; int batch_r, batch_j, batch_g, batch_h; };   // rows and columns of J (m 0: no residual), length of g; lanes per staged sub-batch of each output (0: stored directly)
bool lin_sizes(int kind, LinSizes& s);         // false: unknown or dynamic-size kind
int lin_wave_slab();                           // doubles of LDS a wavefront stages records in
int enqueue_linearize(nlls_ctx* c, const Group& G, int which, int64_t n, const int64_t* d_index, double* d_r, double* d_J, double* d_cost, double* d_g, double* d_H);
// matrix-free products with the linearisation at vars[which] (nlls_apply.hip): device pointers, on c->stream, no synchronisation.  Vector k of v / y starts at k * ndof, of a
// group's u at k * ncost * M.  The caller has checked the arguments (apply_check); nvec is cut into chunks whose records fit nlls_ctx::app_scratch_cap.
int apply_check(nlls_ctx* c, const char* name, int group /* -1: every group */, bool need_residual);     // NLLS_OK, or the status with nlls_last_error set
int enqueue_hess_apply(nlls_ctx* c, int which, double lambda, int nvec, const double* d_v, double* d_y);
int enqueue_jac_apply(nlls_ctx* c, int which, int group, int nvec, const double* d_v, double* d_u);
int enqueue_jact_apply(nlls_ctx* c, int which, int group, int nvec, const double* d_u, double* d_y);
int enqueue_hess_block_diag(nlls_ctx* c, int which, double lambda, double* d_out);
int64_t apply_diag_len(const nlls_ctx* c);     // doubles of nlls_hess_block_diag's output
// block-Jacobi conjugate gradients on (H + c->lambda I) y = b with the products above (nlls_pcg.hip): the caller has checked the arguments and holds b; synchronises once per
// round of c->pcg_round iterations.  NLLS_OK: c->x = -y (and x_out, host, if not null); NLLS_ERR_NOT_SPD: a breakdown, c->x and x_out untouched.  stats: nlls_solve_pcg's (may be null)
int pcg_solve(nlls_ctx* c, int precond, int maxiters, double rtol, double* x_out, double* stats);
// the iteration itself, on ncols right-hand sides, NLLS_APPLY_MAX_VEC at a time: what pcg_solve is one column of, and nlls_solve_pcg_rhs / nlls_marginal_cov call as it is.
// What differs between the three is the call's description.  Exactly one of d_b, B, rows is set:
//   d_b   ONE right-hand side on the device, never written (the step: c->b); the solution leaves as x = -y in c->x, nothing goes to the host, the caller synchronises
//   B     ncols columns of ndof on the host, copied in a batch at a time; `out` (host): the solutions
//   rows  column j is the unit vector of unknown rows[j] (0-based, host), written on the device; `out` (host): rows `rows` of the solutions, ncols x ncols (nlls_marginal_cov)
// Nothing leaves the solver's own buffers -- c->x and `out` stay byte for byte -- before every column of the call has ended well.
struct PcgCall {
    const char* name;                      // the entry point, for the error texts
    int which; double lambda;              // H at this variable set, this damping
    int precond, maxiters; double rtol;
    int64_t ncols;
    const double* d_b = nullptr; const double* B = nullptr; const int64_t* rows = nullptr; double* out = nullptr;
    bool look_first = true;                // the first look at the stop flags before the first product (a zero column, a missing factor pay for none) or behind the first round (one synchronisation less)
    bool schur = false;                    // the operator is S(lambda) of the upload's eliminated set, the vectors have nred entries (d_b only: reduced on the device, the solution expanded there)
    double radius = INFINITY;              // the trust region ||y||_M <= radius (d_b, not schur): a column may then end with status 4 or 5 on the boundary, results like 0 and 1
    double* tr = nullptr;                  // host, two doubles (d_b only): ||y||_M by the recurrence and the model value b'y - 1/2 y'(H + lambda I)y of the column as it ended
};
// NLLS_ERR_NOT_SPD: a column broke down (the error text names the first one).  stats: 4 * ncols + 4 doubles (may be null)
int pcg_solve_cols(nlls_ctx* c, const PcgCall& call, double* stats);
// nlls_solve_pcg_schur: the driver on one column of the reduced system; what pcg_solve does around it, without the phase events and the counters of nlls_get_solve_stats
int pcg_solve_schur(nlls_ctx* c, int precond, int maxiters, double rtol, double* x_out, double* stats);
// nlls_solve_pcg_tr: the driver on pcg_solve's column inside ||y||_M <= radius (Steihaug-Toint), with pcg_solve's transitions and, like pcg_solve_schur, none of its counters
int pcg_solve_tr(nlls_ctx* c, int precond, int maxiters, double rtol, double radius, double* x_out, double* stats);
// Cholesky and inverse, in place, of n diagonal blocks listed by dof and start (nlls_pcg.hip, pcg_factor_kernel): a block without a factor leaves status 3 and the stop flag in scal
int enqueue_block_factor(nlls_ctx* c, const int32_t* d_bsz, const uint32_t* d_dstart, int64_t n, double* d_blocks, double* d_scal);
// what nlls_schur_apply.hip takes from nlls_apply.hip: the index with its row classes, the record scratch for nvec vectors (cut into chunks of `chunk`), the block launch of
// group g on a table of the caller's (where each slot's variable starts in d_in; DEST_NONE: its entries count as 0), records into ApplyIndex::rec
int apply_index(nlls_ctx* c);
struct RowClasses { std::vector<uint32_t> short_rows, long_rows; std::vector<LongItem> items; std::vector<BigRow> big; uint32_t nslots = 0; int part_w_vec = 1, part_w_diag = 1; };
void classify_rows(const nlls_ctx* c, const uint32_t* blocks /* null: all */, size_t n, int64_t wave_min, RowClasses& out);      // the row-class rule of the gathers (needs apply_index)
int enqueue_diag_blocks(nlls_ctx* c, int which);      // every group's diagonal-block records into ApplyIndex::rec, no gather
int apply_records(nlls_ctx* c, int nvec, int& chunk);
int enqueue_hess_blocks(nlls_ctx* c, size_t g, int which, int nvec, const uint32_t* boff, const double* d_in, int64_t in_stride);
// products with S(lambda) = B + lambda I - E (C + lambda I)^-1 E' over the upload's eliminated set (nlls_schur_apply.hip): device pointers, on c->stream, no synchronisation.
// schur_check: NLLS_OK, or the status with nlls_last_error set (what apply_check refuses; nothing eliminated).  schur_prepare builds the r/e index.
enum { SCHUR_APPLY = 0, SCHUR_REDUCE = 1, SCHUR_EXPAND = 2 };
int schur_check(nlls_ctx* c, const char* name);
int schur_prepare(nlls_ctx* c);
// enqueue_schur_setup leaves the inverses of the e blocks of H + lambda I in d_Minv, nlls_hess_block_diag's layout, and status 3 in d_scal where a block has no factor;
// r_blocks says what becomes of the r class: nothing; the blocks of B + lambda I, inverted (block Jacobi); the blocks of S(lambda) (Schur-Jacobi) -- inverted in d_Minv,
// or, with d_sout set, left UNFACTORED in d_sout in nlls_schur_block_diag's layout (SchurJacobiIndex::rstart) while d_Minv holds the e blocks' inverses alone.
enum { SCHUR_R_NONE = 0, SCHUR_R_B = 1, SCHUR_R_S = 2 };
int enqueue_schur_setup(nlls_ctx* c, int which, double lambda, int r_blocks, double* d_Minv, double* d_scal, int64_t* launches, double* d_sout = nullptr);
// the off-diagonal records (nlls_apply.hip, the block launch's fifth mode): sizes per kind, and group g's records at vars[which] to d_out
bool apply_offd_dims(int kind, int& nd, int& od, int* dof /* MAX_SLOTS */);
int enqueue_offd_blocks(nlls_ctx* c, size_t g, int which, double* d_out);
int apply_need_records(nlls_ctx* c, int64_t doubles);      // ApplyIndex::rec holds at least this many
//   SCHUR_APPLY   a = v (nvec x nred)                       out = S v (nvec x nred)
//   SCHUR_REDUCE  a = b (nvec x ndof)                       out = b_r - E (C + lambda I)^-1 b_e (nvec x nred)
//   SCHUR_EXPAND  a = b (nvec x ndof), yr (nvec x nred)     out (nvec x ndof): yr on the r entries, (C + lambda I)^-1 (b_e - E' yr) on the e entries
int enqueue_schur_op(nlls_ctx* c, int mode, int which, double lambda, const double* d_Minv, int nvec, const double* d_a, const double* d_yr, double* d_out);
int enqueue_update_scatter(nlls_ctx* c, Group& G, int64_t n, bool indexed);   // (nlls_update.hip) nlls_set_cost_data: c->upd_stage (blocks c->upd_index) -> every copy of the group's payload
size_t singles_group_size();
void singles_group_fill(void* dst, const Group& G);
int enqueue_quadform(nlls_ctx* c, const double* d_vec, int out_slot /* scalars[out], scalars[out+1] = v'Hv, b'v */);
int enqueue_post_solve(nlls_ctx* c, double* stamps, int retract_to = -1, int retract_from = -1, bool finish = true);
int enqueue_lm_trial_tail(nlls_ctx* c, const TrialArgs& t);   // post-solve statistics + retraction, cost sweep, and ONE finishing launch for both reductions   // enqueue_step_stats + enqueue_quadform(x, 4) for the step of the last solve, fewer launches; optionally the retraction rides along

#if defined(__HIPCC__)
// to[var i] = update(from[var i], x[its block])   (src/linearsystem.jl:206-213); fixed variables are copied
// dx: the variable's own step (its block of x)
// DX(q) = component q of the variable's own step.  No staging arrays with run-time indices (they would live in scratch memory -- 1040 bytes per lane
// of every kernel this is inlined into): Euclidean / dynamic vectors add in place, the other kinds have compile-time sizes.
template <int K, class DXF>
__device__ __forceinline__ void retract_user_var(uint32_t o, const double* __restrict__ from, double* __restrict__ to, DXF DX) {   // a user kind: update<double>, sizes of Var<K>
    constexpr int ST = Var<K>::STORAGE, DF = Var<K>::DOF;
    double in[ST], st[DF], out[ST];
#pragma unroll
    for (int q = 0; q < ST; ++q) in[q] = from[o + q];
#pragma unroll
    for (int q = 0; q < DF; ++q) st[q] = DX(q);
    Var<K>::template update<double>(in, st, out);
#pragma unroll
    for (int q = 0; q < ST; ++q) to[o + q] = out[q];
}
template <class DXF>
__device__ __forceinline__ void retract_var_fn(int k, int d, uint32_t o, const double* __restrict__ from, double* __restrict__ to, DXF DX) {
    switch (k) {
    case NLLS_VAR_EUCLIDEAN: case NLLS_VAR_DYNAMIC: for (int q = 0; q < d; ++q) to[o + q] = from[o + q] + DX(q); return;   // v + delta (src/variable.jl:5): any length
    case NLLS_VAR_ZERO_TO_INF: case NLLS_VAR_ZERO_TO_ONE: { const double in0 = from[o], st0 = DX(0); double out0; var_update_real(k, d, &in0, &st0, &out0); to[o] = out0; return; }
    case NLLS_VAR_CONTAMINATED_GAUSSIAN: { double in[3], st[3], out[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) { in[q] = from[o + q]; st[q] = DX(q); }
        var_update_real(NLLS_VAR_CONTAMINATED_GAUSSIAN, d, in, st, out);
#pragma unroll
        for (int q = 0; q < 3; ++q) to[o + q] = out[q];
        return; }
    case NLLS_VAR_POSE_SO3: { double in[12], st[6], out[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) in[q] = from[o + q];
#pragma unroll
        for (int q = 0; q < 6; ++q) st[q] = DX(q);
        var_update_real(NLLS_VAR_POSE_SO3, d, in, st, out);
#pragma unroll
        for (int q = 0; q < 12; ++q) to[o + q] = out[q];
        return; }
#define X(K) case K: retract_user_var<K>(o, from, to, DX); return;
    NLLS_USER_VAR(X)
#undef X
    }
}
__device__ __forceinline__ void retract_var(int k, int d, uint32_t o, const double* __restrict__ from, const double* __restrict__ dx, double* __restrict__ to) {
    retract_var_fn(k, d, o, from, to, [dx](int q) { return dx[q]; });
}
__device__ __forceinline__ void retract_one(const int32_t* __restrict__ kind, const int32_t* __restrict__ dim, const uint32_t* __restrict__ voff,
                                            const uint32_t* __restrict__ vboff, int64_t i, const double* __restrict__ from,
                                            const double* __restrict__ x, double* __restrict__ to) {
    const int k = kind[i], d = dim[i]; const uint32_t o = voff[i], bo = vboff[i];
    if (bo == DEST_NONE) { const int st = var_storage(k, d); for (int q = 0; q < st; ++q) to[o + q] = from[o + q]; return; }
    retract_var(k, d, o, from, x + bo, to);
}
#endif
// solve (nlls_solve.hip)
int enqueue_solve(nlls_ctx* c, const TrialArgs& t = {});
int enqueue_solve_local(nlls_ctx* c, bool mf = false);
int enqueue_solve_finish(nlls_ctx* c, const TrialArgs& t = {});
int enqueue_tiny_dense_trial(nlls_ctx* c, int to, int from);
int enqueue_tiny_trial_finish_pending(nlls_ctx* c);   // the finishing reduction no accumulate launch has carried   // nlls_ctx::tiny_dense: damped solve + step statistics + retraction in one launch, then the cost sweep
int enqueue_chain_solve(nlls_ctx* c, int n_band, int bw, int nbd, int H);   // the banded reduced system by the chain kernels (nlls_chain.hip)
void chain_form_stats(const nlls_ctx* c, int64_t& form, int64_t& window);   // which chain kernels enqueue_chain_solve launches for this structure (nlls_get_solve_stats [51], [52])
int enqueue_reduced_solve(nlls_ctx* c, bool mf = false);   // the factorisation + backward pass of the assembled reduced system alone (timing)
int enqueue_pack_reduce0(nlls_ctx* c);      // [cost | reduced rows | reduced b] -> redbuf
int enqueue_unpack_reduce0(nlls_ctx* c, bool with_cost = true);


// the matrix-free LM trial (nlls_mf.hip; nlls_ctx::mf_ok)
struct BsfRetract;
int enqueue_mf_solve_local(nlls_ctx* c);
int enqueue_mf_backsub(nlls_ctx* c, const BsfRetract& rt, int write_red, double* zptr, int64_t zcount, unsigned nextra, unsigned nrestwg);
int enqueue_mf_trial_finish(nlls_ctx* c, const TrialArgs& t); int enqueue_mf_trial_finish_now(nlls_ctx* c, const TrialArgs& t); struct MfFin; MfFin mf_fin_args(nlls_ctx* c, double* mirror); size_t mf_part_doubles(int64_t nsupernodes, int64_t nrest_wg_max);
int enqueue_mf_sweep_cost(nlls_ctx* c, int which);   // cost(vars[which]) summed as the matrix-free trial sums its cost
int enqueue_gather(nlls_ctx* c);   // (nlls_solve.hip) schur_gather_kernel: slabs -> the block cyclic reduction's tiles
uint32_t mf_wave_doubles(uint32_t ecap, int dp); int mf_batch_max(); int mf_elim_waves(); uint32_t mf_slab_doubles(int B, int dp, int tr);
int build_mf(nlls_ctx* c, int32_t ngroups, const nlls_cost_group* groups, const uint64_t* bi, int32_t flags);   // (nlls_structure.cpp)
// dynamic LDS above the default for the kernels of the structure just built, on the current device (grant_dynamic_lds; the upload calls them behind build_mf; nlls_bcr.hpp has a fifth)
hipError_t grant_solve_lds(const nlls_ctx* c);   // (nlls_solve.hip) the generic elimination
hipError_t grant_mf_lds(const nlls_ctx* c);      // (nlls_mf.hip) the matrix-free elimination of the group build_mf chose
hipError_t grant_chain_lds(const nlls_ctx* c);   // (nlls_chain.hip) the chain kernels, where they solve the band
hipError_t grant_sweep_lds(const nlls_ctx* c);   // (nlls_sweep.hip) the heavy rows of the accumulate sweep

// collectives (nlls_comm.cpp)
int comm_reduce(nlls_ctx* c, double* dev_ptr, int64_t count, int op);                 // no-op without an installed all-reduce
int comm_gather_trial_scalars(nlls_ctx* c, double seq);                               // gather + combine the trial's scalars on the device, publish them (and seq) to the host mirror
void comm_release(nlls_ctx* c);

inline double* vars_ptr(nlls_ctx* c, int which) { return c->vars[c->vars_slot[which]].p; }

}  // namespace nlls
#include "nlls_state.hpp"
