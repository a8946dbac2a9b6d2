// nlls_pcg.hip -- nlls_solve_pcg: preconditioned conjugate gradients on (H + lambda I) y = b, on the device (gfx950).
//
//   the linear solve of the iterators            src/linearsystem.jl:180-190, src/iterators.jl:149-157 (solve!, negate!)
//
// H is applied by enqueue_hess_apply (nlls_apply.hip) on device pointers -- evaluated at CURRENT, never read from A.data -- and the preconditioner is the inverse of the
// diagonal blocks enqueue_hess_block_diag leaves (block Jacobi), or the identity.  The vector work is three launches per iteration behind the product's:
//   pcg_dot   partials of p'q, one per workgroup
//   pcg_step  alpha = r'z / p'q;  y += alpha p;  r_new = r_old - alpha q (into the OTHER r buffer);  z = Minv r_new;  partials of r'z and r'r
//   pcg_dir   beta = r'z / (r'z of the iteration before);  p = z + beta p;  workgroup 0: the scalars, the iteration counter, the stop test
// Every sum has a fixed order -- a lane's grid-stride terms in index order, block_sum's tree, the partials of all workgroups strided over the lanes of EVERY workgroup
// and the same tree again, so that all workgroups hold the same scalar -- and nothing adds with atomics: two calls on the same b return identical bytes.
// Stop: every kernel of this file returns at entry when PCG_STOP is set, so the iterations the host enqueued behind it (it looks once per round of nlls_ctx::pcg_round
// iterations) cost their launches and the product, and change nothing: the result does not depend on the round length.  The flag is written where the writer's own
// launch cannot be harmed by it: on a breakdown every workgroup takes the same decision and writes nothing; on convergence only p, which nobody reads again, may stay
// partly updated.  Built like nlls_apply.o, WITHOUT -fno-honor-nans: a NaN in b or in a product reaches the breakdown tests below.
// Columns (nlls_solve_pcg_rhs, nlls_marginal_cov): the vector kernels take a column per blockIdx.y -- its own vectors (slot blockIdx.y of each of the six arrays), its
// own scalar block and rows of partials (those of the column PcgArgs::cols names for the slot: a column keeps them when its vectors move to another slot).
// pcg_column() turns the launch's arguments into the column's and the bodies below are those of one column: nlls_solve_pcg launches them with one.  A workgroup
// belongs to one column, so the stop flag is one value per workgroup and a stopped column's workgroups leave at entry while the others iterate.
// Host: ONE driver, pcg_solve_cols, allocates (nlls_ctx::pcg, one set of buffers), fills PcgArgs, launches and loops for the three entry points; a PcgCall
// (nlls_internal.hpp) says where the right-hand sides come from, where a finished column goes and when the first look at the stop flags is due.  pcg_solve is that
// driver on one column -- H at CURRENT, the context's damping, b the gradient where it lies -- plus what is the step's alone: the phase events, step_replaced, the
// counters of nlls_get_solve_stats, the copy to x_out, its eight statistics and its error texts.
// Trust region (nlls_solve_pcg_tr, Steihaug-Toint): the same recurrence, stopped where the iterate would leave ||y||_M <= PcgArgs::radius or where p'q <= 0, and then taken
// to the boundary along p.  M is the preconditioner (the identity without one), the norm in which the iterates grow monotonically, and in exact arithmetic
//   yy = ||y||_M^2   yp = y'Mp   pp = ||p||_M^2        start: 0, 0, r'z;   after alpha: yy += 2 alpha yp + alpha^2 pp;   after beta: yp = beta (yp + alpha pp), pp = r'z_new + beta^2 pp
// follow from scalars the iteration has: no dot product, launch or synchronisation more.  Lane 0 of workgroup 0 of pcg_dir keeps them, with the model value
// b'y - 1/2 y'(H + lambda I)y (+= 1/2 alpha r'z per full step, += tau r'z - 1/2 tau^2 p'q at the boundary), in every call; only a call with a finite radius reads them,
// and with radius = +inf the arithmetic on y, r, z, p is nlls_solve_pcg's operation for operation.  The boundary exit is where the stop-flag rule above bites: EVERY
// workgroup of pcg_step has to write its share of y += tau p, so pcg_step records the exit in PCG_EXIT / PCG_TAU, which no workgroup of its own launch reads, and
// pcg_dir, which then writes no vector, raises the flag and counts the iteration.
#include <algorithm>
#include <cmath>

#include "nlls_wave.hpp"

namespace nlls {

struct PcgArgs {
    const uint32_t* erow; const uint32_t* start; const uint32_t* dstart; const int32_t* bsz;      // ApplyIndex::erow_vec, start_vec, start_diag; nlls_ctx::d_blocksizes
    int64_t ndof, nblocks; int precond, npart, parity;      // npart: workgroups of the vector kernels (= partials per row); parity: of the iteration (which r'z slot is the old one)
    double rtol2;
    const double* b; const double* Minv; double* y; const double* r_old; double* r_new; double* z; double* p; const double* q;
    double* pa; double* pb; double* pc; double* scal;       // partials of p'q, r'z, r'r
    int64_t pstride; uint32_t cols;                         // doubles between two columns' rows of partials; four bits per slot: the column (of the batch) whose scalars and partials it uses
    double radius;                                          // the trust region's, in the norm of M; +inf: none (the three solvers of linear systems)
};
// the arguments of this workgroup's column (everything here is uniform over the workgroup)
NLLS_DEV PcgArgs pcg_column(PcgArgs a) {
    const int64_t v = (int64_t)blockIdx.y * a.ndof, cb = (a.cols >> (4 * blockIdx.y)) & 15u;
    a.b += v; a.y += v; a.r_old += v; a.r_new += v; a.z += v; a.p += v; a.q += v;
    a.pa += cb * a.pstride; a.pb += cb * a.pstride; a.pc += cb * a.pstride; a.scal += cb * PCG_NSCAL;
    return a;
}

// the stop flag as ONE value for the whole workgroup (a barrier follows in every kernel: lanes that read it at different times must not part ways)
NLLS_DEV bool pcg_stopped(const double* scal, double* red) {
    if (threadIdx.x == 0) red[8] = scal[PCG_STOP];
    __syncthreads();
    return red[8] != 0.0;
}
// the same sum of `n` partials in every workgroup: lane t takes t, t + TPB, ... in order, then block_sum's tree; broadcast through red[9]
NLLS_DEV double pcg_total(const double* __restrict__ part, int n, double* red) {
    double s = 0;
    for (int i = (int)threadIdx.x; i < n; i += TPB) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) red[9] = s;
    __syncthreads();
    s = red[9];
    __syncthreads();
    return s;
}
// z[e] = row of the block's inverse times the block's r, r formed by rk(k) for entry k of the block (precond 0: z = r)
template <class RF>
NLLS_DEV double pcg_prec(const PcgArgs& a, int64_t e, double re, RF&& rk) {
    if (!a.precond) return re;
    const uint32_t row = a.erow[e]; const int32_t d = a.bsz[row]; const int64_t s0 = a.start[row];
    const double* __restrict__ m = a.Minv + a.dstart[row] + (int64_t)(e - s0) * d;      // column e - s0 of a symmetric block: contiguous
    double s = 0;
    for (int k = 0; k < d; ++k) s += m[k] * rk(s0 + k);
    return s;
}

// One lane per diagonal block of H + lambda I (column-major dof x dof, as enqueue_hess_block_diag left it): Cholesky, the factor's inverse, the block's inverse, all in
// place, run-time dof up to NLLS_MAX_BLOCK_SZ.  A pivot that is not > 0 (NaN included): status 3 and stop.  Once per solve.
__global__ __launch_bounds__(TPB) void pcg_factor_kernel(PcgArgs a, double* __restrict__ Minv) {
    const int64_t blk = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (blk >= a.nblocks) return;
    const int d = a.bsz[blk]; double* __restrict__ M = Minv + a.dstart[blk];
    bool bad = false;
    for (int j = 0; j < d && !bad; ++j) {                   // M = L L', L in the lower triangle
        double piv = M[j + j * d];
        for (int k = 0; k < j; ++k) piv -= M[j + k * d] * M[j + k * d];
        if (!(piv > 0.0)) { bad = true; break; }
        piv = sqrt(piv); M[j + j * d] = piv;
        for (int i = j + 1; i < d; ++i) { double s = M[i + j * d];
            for (int k = 0; k < j; ++k) s -= M[i + k * d] * M[j + k * d];
            M[i + j * d] = s / piv; }
    }
    if (bad) { a.scal[PCG_STATUS] = 3.0; a.scal[PCG_STOP] = 1.0; return; }      // (every lane that gets here stores the same two values)
    for (int j = 0; j < d; ++j) {                           // L -> L^-1, column by column: rows below and columns right of j still hold L
        M[j + j * d] = 1.0 / M[j + j * d];
        for (int i = j + 1; i < d; ++i) { double s = 0;
            for (int k = j; k < i; ++k) s += M[i + k * d] * M[k + j * d];
            M[i + j * d] = -s / M[i + i * d]; }
    }
    for (int j = 0; j < d; ++j)                             // lower triangle of L^-T L^-1: entry (i, j) needs rows >= i of columns i and j, not yet overwritten
        for (int i = j; i < d; ++i) { double s = 0;
            for (int k = i; k < d; ++k) s += M[k + i * d] * M[k + j * d];
            M[i + j * d] = s; }
    for (int j = 0; j < d; ++j) for (int i = j + 1; i < d; ++i) M[j + i * d] = M[i + j * d];
}

// y = 0, r = b, z = Minv r, p = z; partials of r'z and b'b
__global__ __launch_bounds__(TPB) void pcg_init_kernel(PcgArgs a0) {
    __shared__ double red[16];
    const PcgArgs a = pcg_column(a0);
    if (pcg_stopped(a.scal, red)) return;
    double srz = 0, sbb = 0;
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < a.ndof; e += (int64_t)gridDim.x * TPB) {
        const double re = a.b[e];
        const double ze = pcg_prec(a, e, re, [&](int64_t k) { return a.b[k]; });
        a.y[e] = 0.0; a.r_new[e] = re; a.z[e] = ze; a.p[e] = ze;
        srz += re * ze; sbb += re * re;
    }
    srz = block_sum(srz, red); sbb = block_sum(sbb, red);
    if (threadIdx.x == 0) { a.pb[blockIdx.x] = srz; a.pc[blockIdx.x] = sbb; }
}
// one workgroup: the scalars of the start -- r'z, r'r = b'b; b == 0 (or rtol >= 1) is converged before the first iteration
__global__ __launch_bounds__(TPB) void pcg_start_kernel(PcgArgs a0) {
    __shared__ double red[16];
    const PcgArgs a = pcg_column(a0);
    if (pcg_stopped(a.scal, red)) return;
    const double rz = pcg_total(a.pb, a.npart, red), bb = pcg_total(a.pc, a.npart, red);
    if (threadIdx.x == 0) { a.scal[PCG_RZ0] = rz; a.scal[PCG_RR] = bb; a.scal[PCG_BB] = bb; a.scal[PCG_PP] = rz; if (bb <= a.rtol2 * bb) a.scal[PCG_STOP] = 1.0; }      // (||p||_M^2 = z'Mz = r'z; ||y||_M^2, y'Mp and the model are 0 from pcg_cols_begin_kernel)
}

// ||y + alpha p||_M^2 from the three scalars of the trust region
NLLS_DEV double pcg_yy_next(double yy, double yp, double pp, double alpha) { return fma(alpha, fma(alpha, pp, 2.0 * yp), yy); }

__global__ __launch_bounds__(TPB) void pcg_dot_kernel(PcgArgs a0) {
    __shared__ double red[16];
    const PcgArgs a = pcg_column(a0);
    if (pcg_stopped(a.scal, red)) return;
    double s = 0;
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < a.ndof; e += (int64_t)gridDim.x * TPB) s += a.p[e] * a.q[e];
    s = block_sum(s, red);
    if (threadIdx.x == 0) a.pa[blockIdx.x] = s;
}

__global__ __launch_bounds__(TPB) void pcg_step_kernel(PcgArgs a0) {
    __shared__ double red[16];
    const PcgArgs a = pcg_column(a0);
    if (pcg_stopped(a.scal, red)) return;
    const double pq = pcg_total(a.pa, a.npart, red), rz = a.scal[PCG_RZ0 + a.parity], alpha = rz / pq;
    // The trust region: from scalars every workgroup holds identically (pcg_dir_kernel of the iteration before left them), so all take the same exit.  exit 5: the
    // curvature along p is not positive; exit 4: the full step would leave the ball; either way y goes to the boundary along p, tau the positive root of
    // pp tau^2 + 2 yp tau + (yy - radius^2) = 0 in the form that does not cancel.  A tau that is not a finite step forwards is a breakdown like any other scalar's.
    int ex = 0; double tau = 0.0;
    if (isfinite(a.radius)) {
        const double yy = a.scal[PCG_YY], yp = a.scal[PCG_YP], pp = a.scal[PCG_PP], r2 = a.radius * a.radius;
        if (pq <= 0.0) ex = 5;
        else if (pq > 0.0 && isfinite(alpha) && pcg_yy_next(yy, yp, pp, alpha) >= r2) ex = 4;
        if (ex) { const double d = r2 - yy; tau = d / (yp + sqrt(fma(yp, yp, pp * d))); if (!(isfinite(tau) && tau >= 0.0)) ex = -1; }
    }
    if (ex < 0 || (!ex && (!(pq > 0.0) || !isfinite(alpha)))) {      // the same decision in every workgroup: nobody writes a vector
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.scal[PCG_PQ] = pq; a.scal[PCG_ITER] += 1.0; a.scal[PCG_STATUS] = 2.0; a.scal[PCG_STOP] = 1.0; }
        return;
    }
    const double* __restrict__ ro = a.r_old; const double* __restrict__ q = a.q;
    if (ex) {         // every workgroup writes its share of y += tau p and r_new = r - tau q.  NOT the stop flag: a workgroup of this launch that starts late would find it
                        // at entry and leave its share unwritten -- the exit is recorded in scalars nobody of this launch reads, and pcg_dir_kernel stops the column
        double srr = 0;
        for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < a.ndof; e += (int64_t)gridDim.x * TPB) {
            const double re = fma(-tau, q[e], ro[e]);
            a.y[e] = fma(tau, a.p[e], a.y[e]); a.r_new[e] = re;
            srr += re * re;
        }
        srr = block_sum(srr, red);
        if (threadIdx.x == 0) { a.pc[blockIdx.x] = srr; if (blockIdx.x == 0) { a.scal[PCG_PQ] = pq; a.scal[PCG_TAU] = tau; a.scal[PCG_EXIT] = (double)ex; } }
        return;
    }
    double srz = 0, srr = 0;
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < a.ndof; e += (int64_t)gridDim.x * TPB) {
        const double re = fma(-alpha, q[e], ro[e]);         // (the block's other entries of r_new are formed the same way below: r is never read while it is written)
        const double ze = pcg_prec(a, e, re, [&](int64_t k) { return fma(-alpha, q[k], ro[k]); });
        a.y[e] = fma(alpha, a.p[e], a.y[e]); a.r_new[e] = re; a.z[e] = ze;
        srz += re * ze; srr += re * re;
    }
    srz = block_sum(srz, red); srr = block_sum(srr, red);
    if (threadIdx.x == 0) { a.pb[blockIdx.x] = srz; a.pc[blockIdx.x] = srr; if (blockIdx.x == 0) a.scal[PCG_PQ] = pq; }
}

__global__ __launch_bounds__(TPB) void pcg_dir_kernel(PcgArgs a0) {
    __shared__ double red[16];
    const PcgArgs a = pcg_column(a0);
    if (pcg_stopped(a.scal, red)) return;
    if (a.scal[PCG_EXIT] != 0.0) {      // pcg_step_kernel went to the boundary (every workgroup reads what that launch recorded): the residual there, the model value, the
                                        // iteration, and the stop -- here, where no vector is written any more (p, which nobody reads again, stays as it is)
        const double rr = pcg_total(a.pc, a.npart, red);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const double tau = a.scal[PCG_TAU], pq = a.scal[PCG_PQ], rz = a.scal[PCG_RZ0 + a.parity];
            a.scal[PCG_RR] = rr; a.scal[PCG_ITER] += 1.0; a.scal[PCG_YY] = a.radius * a.radius; a.scal[PCG_MODEL] += tau * rz - 0.5 * tau * tau * pq;
            a.scal[PCG_STATUS] = a.scal[PCG_EXIT]; a.scal[PCG_STOP] = 1.0;
        }
        return;
    }
    const double rz = pcg_total(a.pb, a.npart, red), rr = pcg_total(a.pc, a.npart, red);
    const double beta = rz / a.scal[PCG_RZ0 + a.parity], bb = a.scal[PCG_BB];
    const bool done = rr <= a.rtol2 * bb, bad = !done && !(isfinite(beta) && isfinite(rr));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double rz0 = a.scal[PCG_RZ0 + a.parity], alpha = rz0 / a.scal[PCG_PQ], yp = a.scal[PCG_YP], pp = a.scal[PCG_PP];      // (alpha as pcg_step_kernel formed it)
        a.scal[PCG_YY] = pcg_yy_next(a.scal[PCG_YY], yp, pp, alpha); a.scal[PCG_MODEL] += 0.5 * alpha * rz0;
        a.scal[PCG_YP] = beta * fma(alpha, pp, yp); a.scal[PCG_PP] = fma(beta * beta, pp, rz);
        a.scal[PCG_RZ0 + (a.parity ^ 1)] = rz; a.scal[PCG_RR] = rr; a.scal[PCG_ITER] += 1.0;
        if (done) a.scal[PCG_STOP] = 1.0;
        if (bad) { a.scal[PCG_STATUS] = 2.0; a.scal[PCG_STOP] = 1.0; }
    }
    if (bad) return;
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < a.ndof; e += (int64_t)gridDim.x * TPB) a.p[e] = fma(beta, a.p[e], a.z[e]);
}

// the step: x = -y (src/iterators.jl:151, negate!)
__global__ __launch_bounds__(TPB) void pcg_finish_kernel(const double* __restrict__ y, double* __restrict__ x, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < n; e += (int64_t)gridDim.x * TPB) x[e] = -y[e];
}

// ---- columns: what nlls_solve_pcg_rhs and nlls_marginal_cov add around the kernels above ------------------------------------------------------------------------
// every column's scalar block starts as the factorisation's: zeros, or status 3 and the stop flag -- a block without a factor stops every column of the call
__global__ __launch_bounds__(TPB) void pcg_cols_begin_kernel(const double* __restrict__ fscal, double* __restrict__ scal, int ncol) {
    if ((int)threadIdx.x < ncol * PCG_NSCAL) scal[threadIdx.x] = fscal[threadIdx.x % PCG_NSCAL];
}
// unit right-hand sides written where they are used: column blockIdx.y is e_(rows[blockIdx.y])
__global__ __launch_bounds__(TPB) void pcg_unit_kernel(double* __restrict__ io, int64_t ndof, const int64_t* __restrict__ rows) {
    double* __restrict__ colp = io + (int64_t)blockIdx.y * ndof; const int64_t one = rows[blockIdx.y];
    for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < ndof; e += (int64_t)gridDim.x * TPB) colp[e] = e == one ? 1.0 : 0.0;
}
// the selected rows of the batch's finished columns, one lane per (row, column): cov points at the batch's first column of the m x m block
__global__ __launch_bounds__(TPB) void pcg_pick_kernel(const double* __restrict__ io, int64_t ndof, const int64_t* __restrict__ rows, int64_t m, int ncol, double* __restrict__ cov) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= m * ncol) return;
    const int64_t s = t / m, i = t - s * m;
    cov[s * m + i] = io[s * ndof + rows[i]];
}

// ================================================================================================
// host side
// ================================================================================================
namespace {
// launches of one enqueue_hess_apply of one vector (what it just enqueued: the block launches of the non-empty groups, the gather's)
int64_t product_launches(const nlls_ctx* c) {
    int64_t n = 0; for (const Group& G : c->groups) n += G.ncost > 0;
    return n + (c->info.ndof > 0) + (c->app.nitems > 0) + (c->app.nbig > 0);
}
}  // namespace

// The driver of the three entry points: the only place that allocates, launches and loops.  The caller has checked the arguments.  stats: 4 * ncols + 4 doubles (may be null)
int pcg_solve_cols(nlls_ctx* c, const PcgCall& k, double* stats) {
    constexpr int MAXC = NLLS_APPLY_MAX_VEC;
    const int64_t ndof = k.schur ? c->sch.nred : c->info.ndof, ncols = k.ncols; const int maxiters = k.maxiters; const bool sjacobi = k.schur && k.precond == NLLS_PCG_PRECOND_SCHUR_JACOBI, jacobi = k.precond == NLLS_PCG_PRECOND_BLOCK_JACOBI || sjacobi; const std::string nm(k.name);      // (Schur-Jacobi IS block Jacobi to the seven kernels: only the set-up differs)
    const double* const B = k.B; const bool step = k.d_b != nullptr, units = k.rows != nullptr;
    PcgState& S = c->pcg; const int cap = (int)std::min<int64_t>(ncols, MAXC);
    auto need = [&](auto& buf, size_t n, const char* what) -> int {
        if (buf.n >= n && buf.p) return NLLS_OK;
        const hipError_t e = buf.alloc(n); if (e != hipSuccess) { buf.release(); (void)hipGetLastError(); return hip_fail(c, e, (nm + ": " + what).c_str()); }
        return NLLS_OK; };
    S.pw = std::max<int64_t>((ndof + TPB - 1) / TPB, 1);      // (at least one workgroup and one partial: the vector kernels store theirs unconditionally)
    int rc = need(S.vec, (size_t)(6 * cap * ndof), "the vectors"); if (rc != NLLS_OK) return rc;
    rc = need(S.part, (size_t)(3 * S.pw * cap), "the partial sums"); if (rc != NLLS_OK) return rc;
    rc = need(S.scal, (size_t)((MAXC + 1) * PCG_NSCAL), "the scalars"); if (rc != NLLS_OK) return rc;
    rc = need(S.h_scal, (size_t)(MAXC * PCG_NSCAL), "the pinned mirror of the scalars"); if (rc != NLLS_OK) return rc;
    if (!step) { rc = need(S.io, (size_t)((B ? ncols : (int64_t)cap) * ndof), "the columns"); if (rc != NLLS_OK) return rc; }
    if (jacobi || k.schur) { rc = need(S.Minv, (size_t)std::max<int64_t>(apply_diag_len(c), 1), "the preconditioner's blocks"); if (rc != NLLS_OK) return rc; }
    if (k.schur) { rc = need(c->sch.sred, (size_t)ndof, "the reduced right-hand side"); if (rc != NLLS_OK) return rc;
                   rc = need(c->sch.full, (size_t)c->info.ndof, "the expanded solution"); if (rc != NLLS_OK) return rc; }
    if (units) { rc = need(S.rows, (size_t)ncols, "the selected unknowns"); if (rc != NLLS_OK) return rc;
                 rc = need(S.cov, (size_t)(ncols * ncols), "the covariance block"); if (rc != NLLS_OK) return rc; }
    const int64_t vs = (int64_t)cap * ndof;      // doubles of one of the six arrays: the layout is this call's, whatever an earlier call left in the buffers
    double* const y = S.vec.p; double* const r[2] = {y + vs, y + 2 * vs}; double* const z = y + 3 * vs; double* const p = y + 4 * vs; double* const q = y + 5 * vs;
    double* const fscal = S.scal.p + MAXC * PCG_NSCAL; double* const h = S.h_scal.p;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(S.pw, std::max<int64_t>(c->pcg_grid_max, 1)));
    std::vector<double> st((size_t)(4 * ncols + 4), 0.0);
    int64_t launches = 0, syncs = 0, products = 0, batches = 0; bool bad = false; int64_t bad_col = -1; int bad_status = 0;
    if (units) HIPCHK(hipMemcpyAsync(S.rows.p, k.rows, sizeof(int64_t) * (size_t)ncols, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(fscal, 0, sizeof(double) * PCG_NSCAL, c->stream));
    PcgArgs a{};
    a.ndof = ndof; a.nblocks = (int64_t)c->blocksizes.size(); a.precond = jacobi ? 1 : 0; a.npart = grid; a.parity = 0; a.rtol2 = k.rtol * k.rtol; a.radius = k.radius;
    a.Minv = S.Minv.p; a.y = y; a.r_old = r[1]; a.r_new = r[0]; a.z = z; a.p = p; a.q = q;
    a.pa = S.part.p; a.pb = S.part.p + S.pw; a.pc = S.part.p + 2 * S.pw; a.pstride = 3 * S.pw; a.scal = S.scal.p;
    const double* rhs = k.d_b;
    if (k.schur) {      // the reduced system (the caller has built its index: schur_prepare): the e blocks' inverses -- the operator needs them under either preconditioner -- the
                        // r blocks' under block Jacobi (of B + lambda I) or Schur-Jacobi (of S itself), the reduced layout for the vector kernels, and s = reduce(b) as the
                        // one right-hand side
        rc = enqueue_schur_setup(c, k.which, k.lambda, sjacobi ? SCHUR_R_S : (jacobi ? SCHUR_R_B : SCHUR_R_NONE), S.Minv.p, fscal, &launches); if (rc != NLLS_OK) return rc;
        a.erow = c->sch.erow_r.p; a.start = c->sch.cstart.p; a.dstart = c->app.start_diag.p; a.bsz = c->d_blocksizes.p;
        rc = enqueue_schur_op(c, SCHUR_REDUCE, k.which, k.lambda, S.Minv.p, 1, k.d_b, nullptr, c->sch.sred.p); if (rc != NLLS_OK) return rc; launches += c->sch.launches;
        rhs = c->sch.sred.p;
    } else if (jacobi) {       // the preconditioner: once per call, whatever the number of batches (Minv is this call's: an earlier one left it at its own lambda)
        rc = enqueue_hess_block_diag(c, k.which, k.lambda, S.Minv.p); if (rc != NLLS_OK) return rc; launches += product_launches(c);
        a.erow = c->app.erow_vec.p; a.start = c->app.start_vec.p; a.dstart = c->app.start_diag.p; a.bsz = c->d_blocksizes.p;       // (the index of the products exists: enqueue_hess_block_diag built it)
        PcgArgs f = a; f.scal = fscal;
        hipLaunchKernelGGL(pcg_factor_kernel, dim3((unsigned)((a.nblocks + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, f, S.Minv.p); ++launches;
    }
    const int64_t round = std::max<int64_t>(c->pcg_round, 1);
    for (int64_t j0 = 0; j0 < ncols && bad_status != 3; j0 += MAXC, ++batches) {
        const int nb = (int)std::min<int64_t>(MAXC, ncols - j0);
        double* const bio = B ? S.io.p + j0 * ndof : S.io.p;      // the batch's right-hand sides, then its results (the step has neither here: d_b is read, c->x written at the end)
        if (B) HIPCHK(hipMemcpyAsync(bio, B + j0 * ndof, sizeof(double) * (size_t)(nb * ndof), hipMemcpyHostToDevice, c->stream));
        if (units) { hipLaunchKernelGGL(pcg_unit_kernel, dim3(grid, nb), dim3(TPB), 0, c->stream, bio, ndof, S.rows.p + j0); ++launches; }
        hipLaunchKernelGGL(pcg_cols_begin_kernel, dim3(1), dim3(TPB), 0, c->stream, fscal, S.scal.p, nb);
        a.b = step ? rhs : bio; a.cols = 0x76543210u; a.parity = 0; a.r_old = r[1]; a.r_new = r[0];
        hipLaunchKernelGGL(pcg_init_kernel, dim3(grid, nb), dim3(TPB), 0, c->stream, a);
        hipLaunchKernelGGL(pcg_start_kernel, dim3(1, nb), dim3(TPB), 0, c->stream, a); launches += 3;
        HIPCHK(hipGetLastError());
        int slot_col[MAXC]; for (int s = 0; s < MAXC; ++s) slot_col[s] = s;
        int active = nb; int64_t it = 0;
        auto stopped = [&](int s) { return h[slot_col[s] * PCG_NSCAL + PCG_STOP] != 0.0; };
        auto finalize = [&](int s) -> hipError_t {          // the column's four statistics; its y to its place among the results (the step's one column stays in slot 0).
                                                            // Statuses 4 and 5, the trust region's boundary exits, are results like 0 and 1
            const int col = slot_col[s]; const double* hc = h + col * PCG_NSCAL; double* sc = st.data() + 4 * (j0 + col);
            const int status = hc[PCG_STOP] != 0.0 ? (int)hc[PCG_STATUS] : 1;
            sc[0] = hc[PCG_ITER]; sc[1] = status; sc[2] = std::sqrt(hc[PCG_BB]); sc[3] = std::sqrt(hc[PCG_RR]);
            if (k.tr) { k.tr[0] = std::sqrt(hc[PCG_YY]); k.tr[1] = hc[PCG_MODEL]; }
            if (status == 2 || status == 3) { if (!bad) { bad = true; bad_col = j0 + col; bad_status = status; } if (status == 3) bad_status = 3; return hipSuccess; }
            if (step) return hipSuccess;
            return hipMemcpyAsync(bio + (int64_t)col * ndof, y + (int64_t)s * ndof, sizeof(double) * (size_t)ndof, hipMemcpyDeviceToDevice, c->stream); };
        // a look, then a round.  look_first: the first look finds the columns that need no iteration (b == 0; no factor), so that they pay for no product either; without
        // it the first look comes behind the first round, and the call synchronises once per round and no more
        for (;;) {
            if (it > 0 || k.look_first) {
                HIPCHK(hipMemcpyAsync(h, S.scal.p, sizeof(double) * (size_t)(nb * PCG_NSCAL), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream)); ++syncs;       // one look per round for all columns
                if (it >= maxiters) { for (int s = 0; s < active; ++s) HIPCHK(finalize(s)); active = 0; break; }
                // a stopped column pays for no further product: the columns still iterating stay contiguous -- the last one's y, current r and p move into the freed slot
                // (z, q and the other r are written before they are read in the next iteration)
                int s = 0;
                while (s < active) {
                    if (!stopped(s)) { ++s; continue; }
                    HIPCHK(finalize(s)); int last = --active;
                    while (last > s && stopped(last)) { HIPCHK(finalize(last)); last = --active; }
                    if (last > s) {
                        double* const mv[3] = {y, r[it & 1], p};
                        for (double* v : mv) HIPCHK(hipMemcpyAsync(v + (int64_t)s * ndof, v + (int64_t)last * ndof, sizeof(double) * (size_t)ndof, hipMemcpyDeviceToDevice, c->stream));
                        slot_col[s] = slot_col[last]; ++s;
                    }
                }
                if (active == 0) break;
            }
            const int64_t n = std::min<int64_t>(round, (int64_t)maxiters - it);
            a.cols = 0; for (int s = 0; s < active; ++s) a.cols |= (uint32_t)slot_col[s] << (4 * s);
            for (int64_t i = 0; i < n; ++i, ++it) {
                a.parity = (int)(it & 1); a.r_old = r[it & 1]; a.r_new = r[(it + 1) & 1];
                rc = k.schur ? enqueue_schur_op(c, SCHUR_APPLY, k.which, k.lambda, S.Minv.p, active, p, nullptr, q) : enqueue_hess_apply(c, k.which, k.lambda, active, p, q);
                if (rc != NLLS_OK) return rc;
                hipLaunchKernelGGL(pcg_dot_kernel, dim3(grid, active), dim3(TPB), 0, c->stream, a);
                hipLaunchKernelGGL(pcg_step_kernel, dim3(grid, active), dim3(TPB), 0, c->stream, a);
                hipLaunchKernelGGL(pcg_dir_kernel, dim3(grid, active), dim3(TPB), 0, c->stream, a);
                launches += (k.schur ? c->sch.launches : product_launches(c)) + 3; products += active;
            }
            HIPCHK(hipGetLastError());
        }
        if (units && !bad) { hipLaunchKernelGGL(pcg_pick_kernel, dim3((unsigned)((ncols * nb + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, bio, ndof, S.rows.p, ncols, nb, S.cov.p + j0 * ncols); ++launches;
                             HIPCHK(hipGetLastError()); }
    }
    if (bad_status == 3) for (int64_t j = 0; j < ncols; ++j) { st[4 * j] = 0.0; st[4 * j + 1] = 3.0; st[4 * j + 2] = 0.0; st[4 * j + 3] = 0.0; }   // call-wide: no column started
    if (!bad) {         // every column of the call has ended well: only now does a result leave the solver's own buffers
        const double* yfull = y;
        if (k.schur) { rc = enqueue_schur_op(c, SCHUR_EXPAND, k.which, k.lambda, S.Minv.p, 1, k.d_b, y, c->sch.full.p); if (rc != NLLS_OK) return rc; launches += c->sch.launches; yfull = c->sch.full.p; }
        const int fgrid = (int)std::max<int64_t>(1, std::min<int64_t>((c->info.ndof + TPB - 1) / TPB, std::max<int64_t>(c->pcg_grid_max, 1)));      // (the step has ndof entries on either path)
        if (step) { hipLaunchKernelGGL(pcg_finish_kernel, dim3(fgrid), dim3(TPB), 0, c->stream, yfull, c->x.p, c->info.ndof); ++launches; HIPCHK(hipGetLastError()); }      // (pcg_solve waits for it)
        else {
            // (a batch at a time, as the right-hand sides came: one copy of 16 columns of ba_1kx100k into pageable memory took longer than two of 8, notes/r19.md)
            if (B) { for (int64_t j0 = 0; j0 < ncols; j0 += MAXC) { const int64_t nb = std::min<int64_t>(MAXC, ncols - j0);
                         HIPCHK(hipMemcpyAsync(k.out + j0 * ndof, S.io.p + j0 * ndof, sizeof(double) * (size_t)(nb * ndof), hipMemcpyDeviceToHost, c->stream)); } }
            else HIPCHK(hipMemcpyAsync(k.out, S.cov.p, sizeof(double) * (size_t)(ncols * ncols), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream)); ++syncs;
        }
    }
    double* const tail = st.data() + 4 * ncols;
    tail[0] = (double)syncs; tail[1] = (double)launches; tail[2] = (double)products; tail[3] = (double)batches;
    if (stats) std::copy(st.begin(), st.end(), stats);
    if (bad) {
        c->err = bad_status == 3 ? nm + (k.schur ? ": an eliminated block C_e + lambda I -- or, under block Jacobi, a diagonal block of B + lambda I; under Schur-Jacobi, of S -- is not positive definite (status 3)"
                                                 : ": a diagonal block of H + lambda I is not positive definite (status 3)")
                                 : nm + ": p'(H + lambda I)p is not positive, or a scalar of the recurrence is not finite (status 2, column " + std::to_string(bad_col) + ")";
        return NLLS_ERR_NOT_SPD;
    }
    return NLLS_OK;
}

// the factor launch on a list of blocks of the caller's (nlls_schur_apply.hip: one row class of the reduced layout)
int enqueue_block_factor(nlls_ctx* c, const int32_t* d_bsz, const uint32_t* d_dstart, int64_t n, double* d_blocks, double* d_scal) {
    if (n <= 0) return NLLS_OK;
    PcgArgs f{}; f.nblocks = n; f.bsz = d_bsz; f.dstart = d_dstart; f.scal = d_scal;
    hipLaunchKernelGGL(pcg_factor_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, f, d_blocks);
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}

// nlls_solve_pcg: the driver on ONE column, the gradient where the sweep left it, H at CURRENT under the context's damping -- and what is the step's alone
int pcg_solve(nlls_ctx* c, int precond, int maxiters, double rtol, double* x_out, double* stats) {
    double st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cs[8];         // cs: the column's four statistics, then synchronisations, launches, product vectors, batches
    auto report = [&]() { c->pcg_iters = (int64_t)st[0]; c->pcg_status = (int64_t)st[1]; c->pcg_rounds = (int64_t)st[4]; if (stats) for (int i = 0; i < 8; ++i) stats[i] = st[i]; };
    const bool timed = c->phase_on && c->phase_ev.size() >= 16;
    if (timed) (void)hipEventRecord(c->phase_ev[14], c->stream);
    const int rc = pcg_solve_cols(c, PcgCall{.name = "nlls_solve_pcg", .which = NLLS_VARS_CURRENT, .lambda = c->lambda, .precond = precond, .maxiters = maxiters, .rtol = rtol,
                                             .ncols = 1, .d_b = c->b.p, .look_first = false}, cs);
    if (rc != NLLS_OK && rc != NLLS_ERR_NOT_SPD) return rc;
    for (int i = 0; i < 6; ++i) st[i] = cs[i];
    if (timed) { (void)hipEventRecord(c->phase_ev[15], c->stream); c->pcg_pending = true; }
    if (rc == NLLS_ERR_NOT_SPD) {
        report();
        c->err = (int)st[1] == 3 ? "nlls_solve_pcg: a diagonal block of H + lambda I is not positive definite (status 3)"
                                 : "nlls_solve_pcg: p'(H + lambda I)p is not positive, or a scalar of the recurrence is not finite (status 2, iteration " + std::to_string((int64_t)st[0]) + ")";
        return rc;
    }
    step_replaced(c);
    if (x_out) HIPCHK(hipMemcpyAsync(x_out, c->x.p, sizeof(double) * (size_t)c->info.ndof, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    st[4] += 1.0;
    report();
    return NLLS_OK;
}

// Every unfixed block is eliminated (a bundle adjustment with all cameras fixed): the reduced system has no unknown, there is nothing to iterate on, and the step is
// x = -expand(b, []) = -(C + lambda I)^-1 b -- status 0, no iteration; an eliminated block without a factor is status 3 as elsewhere, the step untouched
static int pcg_solve_schur_empty(nlls_ctx* c, double* x_out, double* stats) {
    PcgState& S = c->pcg; const int64_t ndof = c->info.ndof; double st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, h[PCG_NSCAL]; int64_t launches = 0;
    auto need = [&](DevBuf<double>& buf, size_t n, const char* what) -> int {
        if (buf.n >= n && buf.p) return NLLS_OK;
        const hipError_t e = buf.alloc(n); if (e != hipSuccess) { buf.release(); (void)hipGetLastError(); return hip_fail(c, e, what); }
        return NLLS_OK; };
    int rc = need(S.Minv, (size_t)std::max<int64_t>(apply_diag_len(c), 1), "nlls_solve_pcg_schur: the eliminated blocks' inverses"); if (rc != NLLS_OK) return rc;
    rc = need(S.scal, (size_t)((NLLS_APPLY_MAX_VEC + 1) * PCG_NSCAL), "nlls_solve_pcg_schur: the scalars"); if (rc != NLLS_OK) return rc;
    rc = need(c->sch.full, (size_t)ndof, "nlls_solve_pcg_schur: the expanded solution"); if (rc != NLLS_OK) return rc;
    HIPCHK(hipMemsetAsync(S.scal.p, 0, sizeof(double) * PCG_NSCAL, c->stream));
    rc = enqueue_schur_setup(c, NLLS_VARS_CURRENT, c->lambda, SCHUR_R_NONE, S.Minv.p, S.scal.p, &launches); if (rc != NLLS_OK) return rc;
    rc = enqueue_schur_op(c, SCHUR_EXPAND, NLLS_VARS_CURRENT, c->lambda, S.Minv.p, 1, c->b.p, nullptr, c->sch.full.p); if (rc != NLLS_OK) return rc; launches += c->sch.launches;
    HIPCHK(hipMemcpyAsync(h, S.scal.p, sizeof(double) * PCG_NSCAL, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    st[4] = 1.0; st[5] = (double)launches;
    if (h[PCG_STATUS] != 0.0) { st[1] = 3.0; if (stats) for (int i = 0; i < 8; ++i) stats[i] = st[i];
        c->err = "nlls_solve_pcg_schur: an eliminated block C_e + lambda I is not positive definite (status 3)"; return NLLS_ERR_NOT_SPD; }
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((ndof + TPB - 1) / TPB, std::max<int64_t>(c->pcg_grid_max, 1)));
    hipLaunchKernelGGL(pcg_finish_kernel, dim3(grid), dim3(TPB), 0, c->stream, c->sch.full.p, c->x.p, ndof); HIPCHK(hipGetLastError());
    step_replaced(c);
    if (x_out) HIPCHK(hipMemcpyAsync(x_out, c->x.p, sizeof(double) * (size_t)ndof, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    st[4] = 2.0; st[5] = (double)(launches + 1);
    if (stats) for (int i = 0; i < 8; ++i) stats[i] = st[i];
    return NLLS_OK;
}

// nlls_solve_pcg_schur: the same column on the reduced system -- S yr = reduce(b) from 0, y = expand(b, yr), x = -y -- with pcg_solve's transitions and none of its
// counters or phase events: nlls_get_solve_stats [53..55] and nlls_get_phase_times [14] keep describing the last nlls_solve_pcg
int pcg_solve_schur(nlls_ctx* c, int precond, int maxiters, double rtol, double* x_out, double* stats) {
    double st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cs[8];
    int rc = schur_prepare(c); if (rc != NLLS_OK) return rc;
    if (c->sch.nred == 0) return pcg_solve_schur_empty(c, x_out, stats);
    rc = pcg_solve_cols(c, PcgCall{.name = "nlls_solve_pcg_schur", .which = NLLS_VARS_CURRENT, .lambda = c->lambda, .precond = precond, .maxiters = maxiters, .rtol = rtol,
                                   .ncols = 1, .d_b = c->b.p, .look_first = false, .schur = true}, cs);
    if (rc != NLLS_OK && rc != NLLS_ERR_NOT_SPD) return rc;
    for (int i = 0; i < 6; ++i) st[i] = cs[i];
    if (rc == NLLS_OK) {
        step_replaced(c);
        if (x_out) HIPCHK(hipMemcpyAsync(x_out, c->x.p, sizeof(double) * (size_t)c->info.ndof, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        st[4] += 1.0;
    }
    if (stats) for (int i = 0; i < 8; ++i) stats[i] = st[i];
    return rc;
}

// nlls_solve_pcg_tr: pcg_solve's column -- H at CURRENT, the context's damping, the gradient where it lies -- inside ||y||_M <= radius, with pcg_solve's transitions and,
// like pcg_solve_schur, none of its counters or phase events.  The six statistics of pcg_solve, then ||y||_M and the predicted reduction: on a boundary exit the norm IS
// the radius (the recurrence's value there is radius^2 by construction)
int pcg_solve_tr(nlls_ctx* c, int precond, int maxiters, double rtol, double radius, double* x_out, double* stats) {
    double st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cs[8], tr[2] = {0, 0};
    const int rc = pcg_solve_cols(c, PcgCall{.name = "nlls_solve_pcg_tr", .which = NLLS_VARS_CURRENT, .lambda = c->lambda, .precond = precond, .maxiters = maxiters, .rtol = rtol,
                                             .ncols = 1, .d_b = c->b.p, .look_first = false, .radius = radius, .tr = tr}, cs);
    if (rc != NLLS_OK && rc != NLLS_ERR_NOT_SPD) return rc;
    for (int i = 0; i < 6; ++i) st[i] = cs[i];
    if (rc == NLLS_OK) {
        step_replaced(c);
        if (x_out) HIPCHK(hipMemcpyAsync(x_out, c->x.p, sizeof(double) * (size_t)c->info.ndof, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        st[4] += 1.0;
        st[6] = (int)st[1] >= 4 ? radius : tr[0]; st[7] = tr[1];
    }
    if (stats) for (int i = 0; i < 8; ++i) stats[i] = st[i];
    return rc;
}

}  // namespace nlls
