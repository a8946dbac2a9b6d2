// nlls_cost.hip -- cost sweep, retraction, step statistics and optimizesingles! (gfx950).
//
//   cost(vars, costs)                     src/cost.jl:10-13 -> src/residual.jl:49-55
//   update!(to, from, linsystem)          src/linearsystem.jl:206-213
//   optimizesingles!                      src/optimize.jl:60-76,183-205
//
// Built WITHOUT the -fno-honor-nans / -fno-signed-zeros flags of nlls_sweep.hip: the NaN / Inf behaviour of these kernels is part of
// the reference's semantics (a NaN cost is accepted by '!(cost > bestcost)', the termination flags report non-finite costs and steps).
#include <cstring>
#include <utility>

#include "nlls_wave.hpp"
#include "nlls_post.hpp"

namespace nlls {

// ================================================================================================
// cost sweep   src/cost.jl:10-13 -> src/residual.jl:49-55
// ================================================================================================
// POST: the workgroups in front of the last `cgrid` carry the step-statistics roles of an LM trial (nlls_post.hpp: quadratic form, g'x, max |x| of the step the
// back-substitution in front of this launch has just formed -- independent of the cost blocks, and a launch of their own would cost more than they do)
template <int KIND, bool POST>
__global__ __launch_bounds__(TPB) void cost_kernel(const double* __restrict__ vars, const double* __restrict__ data,
                                                   const uint32_t* __restrict__ voff, const uint32_t* __restrict__ index,
                                                   int64_t n, RobustSpec rk, double* __restrict__ partials, int cgrid, PostSolveArgs post) {
    using R = Res<KIND>;
    // (the roles come FIRST in the grid: their chains of dependent loads are the longer ones, and the cost blocks alone fill every wave slot of the chip --
    //  behind them the roles would only start when the sweep is over)
    int bid = (int)blockIdx.x;
    if constexpr (POST) { if (blockIdx.x == 0 && threadIdx.x == 0) time_stamp(post.stamps, 2);
        const int npost = (int)gridDim.x - cgrid; if (bid < npost) { post_roles_any(post, bid); return; } bid -= npost; }
    __shared__ double red[TPB / 64];
    double acc = 0;
    for (int64_t i = (int64_t)bid * TPB + threadIdx.x; i < n; i += (int64_t)cgrid * TPB) {
        const int64_t k = index ? index[i] : i;
        double d[R::NDATA]; uint32_t vo[R::NDEPS];
#pragma unroll
        for (int q = 0; q < R::NDATA; ++q) d[q] = data[k * R::NDATA + q];
#pragma unroll
        for (int q = 0; q < R::NDEPS; ++q) vo[q] = voff[k * R::NDEPS + q];
        acc += block_cost<KIND>(vars, vo, d, rk);
    }
    double t = block_sum(acc, red);
    if (threadIdx.x == 0) partials[bid] = t;
}

// final deterministic reduction of the per-workgroup partials
__global__ __launch_bounds__(TPB) void reduce_partials_kernel(const double* __restrict__ partials, int64_t n, double* __restrict__ out) {
    __shared__ double red[TPB / 64];
    reduce_partials_body(partials, n, out, red);
}

// ================================================================================================
// dynamic-size residual blocks   computeresjacdynamic, src/autodiff.jl:96-121 (heap-allocated, run-time sizes in the reference)
// The registered residuals have closed-form Jacobians: LinearResidual X'w - y (test/dynamicvars.jl:3-11), J = X'; NormResidual w
// (test/dynamicvars.jl:13-21), J = I.  One workgroup per block; n = the variable's run-time length.  With A != nullptr the block's
// J'J and J'r go into the dense linear system (src/residual.jl:72-74, src/linearsystem.jl:132-175), else only the cost.
// ================================================================================================
// Under a robust kernel rho (round 3): cost = rho(r'r) / 2, g = rho' J'r, H = rho' J'J + 2 rho'' (J'r)(J'r)'   (src/residual.jl:76-101 applies to any
// residual, the dynamic ones included); the non-squared cost kind takes none.
__global__ __launch_bounds__(TPB) void dyn_block_kernel(int kind, int n, int ndata, const double* __restrict__ vars, const double* __restrict__ data,
                                                        const uint32_t* __restrict__ voff, const uint32_t* __restrict__ index, const uint32_t* __restrict__ brow,
                                                        int ndof, double* __restrict__ A, double* __restrict__ b, double* __restrict__ partials, RobustSpec rk,
                                                        const uint32_t* __restrict__ aoff = nullptr) {
    __shared__ double red[TPB / 64]; __shared__ double total;
    const int64_t k = index ? index[blockIdx.x] : blockIdx.x;
    const double* w = vars + voff[k];
    const uint32_t bo = (A && brow) ? brow[blockIdx.x] : DEST_NONE;            // (brow is in launch order: one entry per launched block)
    // where H(i, j) of the block goes: the dense system (lower triangle: mirrored behind the sweep), or -- aoff -- the variable's n x n diagonal block of a
    // block-sparse system, which is stored in full (src/linearsystem.jl:140)
    const bool blk = aoff != nullptr; const size_t abase = blk ? (size_t)aoff[blockIdx.x] : 0;
    auto Hat = [&](int i, int j) -> double* { return blk ? A + abase + i + (size_t)n * j : A + (bo + i) + (size_t)ndof * (bo + j); };
    const bool robust = (rk.kind & 0xF) != NLLS_ROBUST_NONE || (rk.kind & NLLS_ROBUST_SCALED);
    double cost;
    // rho, rho', rho'' at c = r'r (every thread: c is the workgroup's total)
    auto kernel_at = [&](double c, double& rho, double& d1, double& d2) { if (robust) robustifydcost_fixed(rk, c, rho, d1, d2); else { rho = c; d1 = 1.0; d2 = 0.0; } };
    if (kind == NLLS_RES_DYN_LINEAR) {
        const double* dd = data + k * (int64_t)ndata; const double* X = dd + 1;
        double acc = 0;
        for (int i = threadIdx.x; i < n; i += TPB) acc += X[i] * w[i];
        { const double t = block_sum(acc, red); if (threadIdx.x == 0) total = t; }   // (block_sum leaves the total in thread 0)
        __syncthreads();
        const double r = total - dd[0];
        double rho, d1, d2; kernel_at(r * r, rho, d1, d2);
        cost = 0.5 * rho;
        if (bo != DEST_NONE) {
            const double hs = d1 + 2.0 * d2 * r * r;                             // J'J = X X', J'r = X r: H = (rho' + 2 rho'' r^2) X X'
            for (int i = threadIdx.x; i < n; i += TPB) atomicAdd(&b[bo + i], d1 * (X[i] * r));
            for (int64_t e = threadIdx.x; e < (int64_t)n * n; e += TPB) { const int i = (int)(e % n), j = (int)(e / n); if (i >= j || blk) atomicAdd(Hat(i, j), hs * (X[i] * X[j])); }
        }
    } else if (kind == NLLS_RES_DYN_LINEARSQ) {                                   // X*w - y, X square (n <= 512): J = X
        __shared__ double rs[512], gs[512];
        const double* dd = data + k * (int64_t)ndata; const double* X = dd + n;
        for (int i = threadIdx.x; i < n; i += TPB) { double t = -dd[i]; for (int j = 0; j < n; ++j) t = fma(X[i + (size_t)n * j], w[j], t); rs[i] = t; }
        __syncthreads();
        double acc = 0;
        for (int i = threadIdx.x; i < n; i += TPB) acc += rs[i] * rs[i];
        { const double t = block_sum(acc, red); if (threadIdx.x == 0) total = t; }
        __syncthreads();
        double rho, d1, d2; kernel_at(total, rho, d1, d2);
        cost = 0.5 * rho;
        if (bo != DEST_NONE) {
            for (int j = threadIdx.x; j < n; j += TPB) { double t = 0; for (int i = 0; i < n; ++i) t = fma(X[i + (size_t)n * j], rs[i], t); gs[j] = t; atomicAdd(&b[bo + j], d1 * t); }
            __syncthreads();
            for (int64_t e = threadIdx.x; e < (int64_t)n * n; e += TPB) { const int j = (int)(e % n), q = (int)(e / n); if (j < q && !blk) continue;
                double h = 0; for (int i = 0; i < n; ++i) h = fma(X[i + (size_t)n * j], X[i + (size_t)n * q], h);
                atomicAdd(Hat(j, q), robust ? d1 * h + (2.0 * d2 * gs[j]) * gs[q] : h); }
        }
    } else if (kind == NLLS_COST_DYN_LINEAR) {                                   // non-squared cost y'w: value, gradient y, Hessian 0
        const double* y = data + k * (int64_t)ndata;
        double acc = 0;
        for (int i = threadIdx.x; i < n; i += TPB) acc += y[i] * w[i];
        cost = block_sum(acc, red);
        if (bo != DEST_NONE) for (int i = threadIdx.x; i < n; i += TPB) atomicAdd(&b[bo + i], y[i]);
    } else {                                                                      // NormResidual w: J = I
        double acc = 0;
        for (int i = threadIdx.x; i < n; i += TPB) acc += w[i] * w[i];
        { const double t = block_sum(acc, red); if (threadIdx.x == 0) total = t; }
        __syncthreads();
        double rho, d1, d2; kernel_at(total, rho, d1, d2);
        cost = 0.5 * rho;
        if (bo != DEST_NONE) {
            for (int i = threadIdx.x; i < n; i += TPB) { atomicAdd(&b[bo + i], d1 * w[i]); if (!robust || d2 == 0.0) atomicAdd(Hat(i, i), d1); }
            if (robust && d2 != 0.0)                                                // H = rho' I + 2 rho'' w w'
                for (int64_t e = threadIdx.x; e < (int64_t)n * n; e += TPB) { const int i = (int)(e % n), j = (int)(e / n); if (i >= j || blk) atomicAdd(Hat(i, j), (i == j ? d1 : 0.0) + (2.0 * d2 * w[i]) * w[j]); }
        }
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = cost;
}

// ================================================================================================
// vector helpers
// ================================================================================================
// update!(to, from, linsystem)   src/linearsystem.jl:206-213
__global__ void retract_kernel(const int32_t* __restrict__ kind, const int32_t* __restrict__ dim, const uint32_t* __restrict__ voff,
                               const uint32_t* __restrict__ vboff, int64_t nvar, const double* __restrict__ from,
                               const double* __restrict__ x, double* __restrict__ to) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nvar) retract_one(kind, dim, voff, vboff, i, from, x, to);
}
// maximum(abs, x) and x'x   (src/optimize.jl:149, src/iterators.jl:160; NaN propagates like Julia's maximum).
// Two stages: per-workgroup partials (max, nan flag, sum of squares), then one small finishing workgroup.
constexpr int RED_BLOCKS = 256;
__global__ __launch_bounds__(TPB) void step_stats_partial_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ part) {
    __shared__ double red[TPB / 64];
    double m = 0, s = 0; bool nan = false;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) { double v = x[i]; nan |= is_nan_bits(v); m = fmax(m, fabs(v)); s += v * v; }
    double mm = block_max(m, red);
    double ss = block_sum(s, red);
    double nn = block_max(nan ? 1.0 : 0.0, red);
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = mm; part[3 * blockIdx.x + 1] = nn; part[3 * blockIdx.x + 2] = ss; }
}
__global__ __launch_bounds__(TPB) void step_stats_finish_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
    __shared__ double red[TPB / 64];
    double m = 0, s = 0, nn = 0;
    for (int i = threadIdx.x; i < nb; i += TPB) { m = fmax(m, part[3 * i]); nn = fmax(nn, part[3 * i + 1]); s += part[3 * i + 2]; }
    double mm = block_max(m, red); double ss = block_sum(s, red); double n2 = block_max(nn, red);
    if (threadIdx.x == 0) { out[1] = n2 > 0 ? __longlong_as_double(0x7ff8000000000000LL) : mm; out[2] = ss; }
}
// initlambda's max |H_ii|   src/iterators.jl:131-137
__global__ __launch_bounds__(TPB) void max_abs_diag_partial_kernel(const double* __restrict__ A, const int64_t* __restrict__ diag_off,
                                                                   const int32_t* __restrict__ bs, const uint8_t* __restrict__ rowmask, int64_t nb, int64_t ld_dense, double* __restrict__ part) {
    __shared__ double red[TPB / 64];
    double m = 0; bool nan = false;
    for (int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x; k < nb; k += (int64_t)gridDim.x * TPB) {
        const int n = bs[k]; const int64_t o = diag_off[k]; const int64_t ld = ld_dense ? ld_dense : n;
        if (o < 0 || (rowmask && !rowmask[k])) continue;
        for (int i = 0; i < n; ++i) { const double a = A[o + i + ld * i]; nan |= is_nan_bits(a); m = fmax(m, fabs(a)); }
    }
    double mm = block_max(m, red);
    double nn = block_max(nan ? 1.0 : 0.0, red);             // Julia's max propagates NaN (src/iterators.jl:131-137): so does this
    if (threadIdx.x == 0) part[blockIdx.x] = nn > 0 ? __longlong_as_double(0x7ff8000000000000LL) : mm;
}
__global__ __launch_bounds__(TPB) void max_finish_kernel(const double* __restrict__ part, int nb, double* __restrict__ out, int slot) {
    __shared__ double red[TPB / 64];
    double m = 0;
    bool nan = false;
    for (int i = threadIdx.x; i < nb; i += TPB) { nan |= is_nan_bits(part[i]); m = fmax(m, part[i]); }
    double mm = block_max(m, red);
    double nn = block_max(nan ? 1.0 : 0.0, red);
    if (threadIdx.x == 0) out[slot] = nn > 0 ? __longlong_as_double(0x7ff8000000000000LL) : mm;
}

// ================================================================================================
// optimizesingles!(problem, options, indices)   src/optimize.jl:60-76,183-205
// Every listed variable is optimised on its own -- all other variables fixed -- against the cost blocks that depend on
// it: the whole outer loop (src/optimize.jl:109-180) with the Levenberg-Marquardt iterator (src/iterators.jl:139-172) and
// the univariate linear system (src/linearsystem.jl:12-32,126-130) runs in ONE thread per variable -- or with the Newton, dogleg or
// gradient-descent iterator (src/iterators.jl:15-27,47-115,187-208); the subproblems of one launch are independent (no cost block
// holds two of them: listed variables that share a block are relaxed one after the other, in launches of independent sets).
// ================================================================================================
struct SinglesGroup { int kind; const double* data; const uint32_t* voff; RobustSpec rk; };
struct SinglesOpt { int maxiters, maxfails; double reldcost, absdcost, dstep; int iterator; };   // iterator: 0 Newton, 1 Levenberg-Marquardt, 2 dogleg, 3 gradient descent
constexpr int SGL_MAXD = 6;                                   // dof of a variable the thread kernel takes
constexpr int SGL_WAVE_MAXD = NLLS_SINGLES_MAX_DOF;           // dof of a variable the wavefront kernel takes (MAXST: every fixed-size kind)
static_assert(SGL_WAVE_MAXD <= MAXST && SGL_MAXD <= SGL_WAVE_MAXD);

// What one subproblem keeps between its evaluations: the sums over its blocks (g, H in full, column-major with stride MAXD), the step, the factor.  The thread kernel has
// one per lane in private memory.  The wavefront kernel has one per wavefront in LDS: its 64 lanes hold identical values, and arrays that the solver indexes at run time
// would otherwise live in scratch memory (12 dof: 90 doubles of sums, as many of the factor).
template <int MAXD> struct SinglesWork { double g[MAXD], H[MAXD * MAXD], x[MAXD], Ld[MAXD * MAXD], y[MAXD], cauchy[MAXD]; };
// a loop over a variable's storage: the wavefront kernel keeps the three points of the subproblem in registers, so its loops are unrolled under a wave-uniform guard
#define SGL_FOR_ST(q) _Pragma("unroll") for (int q = 0; q < (WAVE ? MAXST : ns); ++q) if (!WAVE || q < ns)

// one cost block of the subproblem: the variable's storage comes from `vloc`, everything else from `vars`
template <int KIND, int MAXD, bool WAVE>
NLLS_DEV void singles_block(const SinglesGroup& G, uint32_t k, int slot, const double* __restrict__ vars, const double* vloc,
                            bool want_gh, double& cost, double* g, double* H) {
    using R = Res<KIND>; using I = ResInfo<KIND>;
    double d[R::NDATA]; uint32_t vo[R::NDEPS];
#pragma unroll
    for (int q = 0; q < R::NDATA; ++q) d[q] = G.data[(size_t)k * R::NDATA + q];
#pragma unroll
    for (int q = 0; q < R::NDEPS; ++q) vo[q] = G.voff[(size_t)k * R::NDEPS + q];
    double st[R::NDEPS][MAXST];
    BlockGH<KIND>::load(vars, vo, st);
    static_for<R::NDEPS>([&](auto Sc) {
        constexpr int S = decltype(Sc)::value;
        if (S == slot) {
#pragma unroll
            for (int q = 0; q < I::sto(S); ++q) st[S][q] = vloc[q];
        }
    });
    BlockGH<KIND> B; B.compute_st(st, d, G.rk, false);        // an adaptive kernel variable stays fixed (it is not the one being optimised)
    cost += B.cost;
    if (!want_gh) return;
    static_for<R::NDEPS>([&](auto Sc) {
        constexpr int S = decltype(Sc)::value;
        constexpr int DS = I::dof(S);
        if constexpr (DS > MAXD) return;                      // (a wider slot never reaches this kernel: nlls_optimize_singles)
        else if constexpr (WAVE) {
            // (no branch on the slot around these stores: the compiler merges the ends of such branches into ONE store through a selected address, and an array whose
            //  address is selected at run time stays in scratch memory)
            const bool mine = S == slot;
#pragma unroll
            for (int j = 0; j < DS; ++j) {
                g[j] += mine ? g_elem<KIND, S>(B, j) : 0.0;
#pragma unroll
                for (int i = j; i < DS; ++i) H[i + MAXD * j] += mine ? h_elem<KIND, S, S>(B, i, j) : 0.0;
            }
        } else {
            if (S == slot) {
#pragma unroll
                for (int j = 0; j < DS; ++j) {
                    g[j] += g_elem<KIND, S>(B, j);
#pragma unroll
                    for (int i = 0; i < DS; ++i) H[i + MAXD * j] += h_elem<KIND, S, S>(B, i, j);
                }
            }
        }
    });
}

// update(var, step) without a run-time index into the wavefront kernel's per-lane arrays: var_update_real, the kind a constant in every call
template <int MAXD>
NLLS_DEV void singles_update_static(int kind, int dim, const double* in, const double* d, double* out) {
    switch (kind) {
    case NLLS_VAR_EUCLIDEAN:
#pragma unroll
        for (int i = 0; i < MAXD; ++i) if (i < dim) out[i] = in[i] + d[i];
        break;
#define X(K) case K: if constexpr (var_dof(K, 0) <= MAXD) var_update_real(K, dim, in, d, out); break;
    X(NLLS_VAR_ZERO_TO_INF) X(NLLS_VAR_ZERO_TO_ONE) X(NLLS_VAR_CONTAMINATED_GAUSSIAN) X(NLLS_VAR_POSE_SO3) NLLS_USER_VAR(X)
#undef X
    }
}

// The subproblem of ONE variable, from the point in vcur: src/optimize.jl:109-180 with the iterators of src/iterators.jl.  evaluate(vloc, want_gh) returns the cost at
// vloc and, with want_gh, leaves the gradient and the Hessian (both triangles) in w.g and w.H.  The result is left in vcur; returns the iterations taken.  The thread
// kernel runs it in one lane; the wavefront kernel in all 64 in lockstep on identical sums: every branch in here is wave-uniform, and every store to `w` is the same
// value from every lane.
template <int MAXD, bool WAVE, class Eval>
NLLS_DEV int singles_iterate(const int kind, const int dim, const int nd, const int ns, const SinglesOpt& opt, double* vcur, SinglesWork<MAXD>& w, Eval&& evaluate) {
    double* const g = w.g; double* const H = w.H; double* const x = w.x; double* const cauchy = w.cauchy;
    double vnext[MAXST], vbest[MAXST];
    SGL_FOR_ST(q) vbest[q] = vcur[q];
    double bestcost = evaluate(vcur, true), cost = bestcost;   // src/optimize.jl:118
    double lambda = 0.0, trust = 0.0, stepsize = 1.0;          // reset!(iteratedata): every subproblem starts from the iterator's initial state
    int fails = 0, iter = 0;
    // (H + lam I) x = -g by LDL' (the univariate system; src/linearsolver.jl:20-32)
    auto solve = [&](double lam) {
        double* const Ld = w.Ld; double* const y = w.y;
        for (int j = 0; j < nd; ++j) for (int i = j; i < nd; ++i) Ld[i + MAXD * j] = H[i + MAXD * j] + (i == j ? lam : 0.0);
        for (int j = 0; j < nd; ++j) {
            double dj = Ld[j + MAXD * j];
            for (int k = 0; k < j; ++k) dj -= Ld[j + MAXD * k] * Ld[j + MAXD * k] * Ld[k + MAXD * k];
            Ld[j + MAXD * j] = dj;
            for (int i = j + 1; i < nd; ++i) { double s2 = Ld[i + MAXD * j];
                for (int k = 0; k < j; ++k) s2 -= Ld[i + MAXD * k] * Ld[j + MAXD * k] * Ld[k + MAXD * k];
                Ld[i + MAXD * j] = s2 / dj; }
        }
        for (int i = 0; i < nd; ++i) { double s2 = g[i];
            for (int k = 0; k < i; ++k) s2 -= Ld[i + MAXD * k] * y[k];
            y[i] = s2; }
        for (int i = 0; i < nd; ++i) y[i] /= Ld[i + MAXD * i];
        for (int i = nd - 1; i >= 0; --i) { double s2 = y[i]; for (int k = i + 1; k < nd; ++k) s2 -= Ld[k + MAXD * i] * y[k]; y[i] = s2; }
        for (int i = 0; i < nd; ++i) x[i] = -y[i];                                  // negate!
    };
    auto maxabs_x = [&]() { double m = 0; for (int i = 0; i < nd; ++i) m = is_nan_bits(x[i]) ? x[i] : (is_nan_bits(m) ? m : fmax(m, fabs(x[i]))); return m; };
    auto trial = [&]() {                                                       // update! + cost(varnext)
        if constexpr (WAVE) singles_update_static<MAXD>(kind, dim, vcur, x, vnext); else var_update_real(kind, dim, vcur, x, vnext);
        return evaluate(vnext, false); };
    auto quad = [&](const double* u) { double q = 0; for (int j = 0; j < nd; ++j) for (int i = 0; i < nd; ++i) q += u[i] * H[i + MAXD * j] * u[j]; return q; };   // fast_bAb
    while (true) {
        ++iter;
        double maxstep = 0;
        if (opt.iterator == 0) {
            // ---- iterate!(NewtonData)   src/iterators.jl:15-27
            solve(0.0); cost = trial();
        } else if (opt.iterator == 1) {
            // ---- iterate!(LevMarData)   src/iterators.jl:139-172
            if (lambda == 0.0) { double m = 0; for (int i = 0; i < nd; ++i) m = fmax(m, fabs(H[i + MAXD * i])); lambda = m * 1e-6; }
            double mu = 2.0;
            while (true) {
                solve(lambda);                                                     // :149-153
                const double cost_ = trial();                                      // :155-157
                if (!(cost_ > bestcost) || maxabs_x() < opt.dstep) {               // :160
                    double gx = 0;                                                 // fast_bAb(H, x), dot(g, x) on the undamped H  :162-163
                    for (int j = 0; j < nd; ++j) gx += g[j] * x[j];
                    const double q = (cost_ - bestcost) / (0.5 * quad(x) + gx);
                    lambda *= q < 0.983 ? 1.0 - (2.0 * q - 1.0) * (2.0 * q - 1.0) * (2.0 * q - 1.0) : 0.1;   // :164
                    cost = cost_;
                    break;
                }
                lambda *= mu; mu *= 2.0;                                           // :169-170
                if (!(lambda < 1e300)) { cost = cost_; break; }                    // (a block that never improves: leave instead of spinning)
            }
        } else if (opt.iterator == 2) {
            // ---- iterate!(DoglegData)   src/iterators.jl:47-115
            double gnorm2 = 0; for (int i = 0; i < nd; ++i) gnorm2 += g[i] * g[i];
            const double a = gnorm2 / (quad(g) + 2.2250738585072014e-308);         // floatmin
            for (int i = 0; i < nd; ++i) cauchy[i] = -a * g[i];
            const double alpha2 = a * a * gnorm2, alpha = sqrt(alpha2); double beta = 0;
            if (trust == 0.0) trust = alpha;                                       // first step: the Cauchy point
            if (alpha < trust) { solve(0.0); double s2 = 0; for (int i = 0; i < nd; ++i) s2 += x[i] * x[i]; beta = sqrt(s2); }
            double cost_ = bestcost; int spins = 0;
            while (true) {
                double linear_approx;
                if (!(alpha < trust)) { for (int i = 0; i < nd; ++i) x[i] = (trust / alpha) * cauchy[i]; linear_approx = trust * (2 * alpha - trust) / (2 * a); }
                else if (beta <= trust) linear_approx = cost_;
                else {
                    double sq_leg = 0, c = 0;
                    for (int i = 0; i < nd; ++i) { x[i] -= cauchy[i]; sq_leg += x[i] * x[i]; c += cauchy[i] * x[i]; }
                    const double trsq = trust * trust - alpha2; double step = sqrt(c * c + sq_leg * trsq);
                    step = c <= 0 ? (-c + step) / sq_leg : trsq / (c + step);
                    for (int i = 0; i < nd; ++i) x[i] = x[i] * step + cauchy[i];
                    linear_approx = 0.5 * (a * (1 - step) * (1 - step) * gnorm2) + step * (2 - step) * cost_;
                }
                cost_ = trial();
                const double mu = (bestcost - cost_) / linear_approx;
                if (mu > 0.375) { double s2 = 0; for (int i = 0; i < nd; ++i) s2 += x[i] * x[i]; trust = fmax(trust, 3 * sqrt(s2)); }
                else if (mu < 0.125) trust *= 0.5;
                if (!(cost_ > bestcost) || maxabs_x() < opt.dstep || ++spins > 2000) break;
            }
            cost = cost_;
        } else {
            // ---- iterate!(GradientDescentData)   src/iterators.jl:187-208
            for (int i = 0; i < nd; ++i) x[i] = -g[i] * stepsize;
            double costc = trial(); int spins = 0;
            while (costc > bestcost && ++spins <= 2000) {
                double coststep = 0; for (int i = 0; i < nd; ++i) coststep += x[i] * g[i];
                const double costdiff = bestcost + coststep - costc;
                stepsize *= 0.5 * coststep / costdiff;
                for (int i = 0; i < nd; ++i) x[i] = -g[i] * stepsize;
                costc = trial();
            }
            stepsize *= 2; cost = costc;
        }
        maxstep = maxabs_x();
        // ---- src/optimize.jl:128-160
        double dcost = bestcost - cost;
        if (dcost >= 0) { bestcost = cost; fails = 0; }
        else { dcost = cost; ++fails; if (fails == 1) SGL_FOR_ST(q) vbest[q] = vcur[q]; }
        SGL_FOR_ST(q) vcur[q] = vnext[q];                           // updatefromnext!
        int conv = 0;
        conv |= (fabs(cost) == INFINITY) << 0; conv |= (int)is_nan_bits(cost) << 1;
        conv |= (dcost < bestcost * opt.reldcost) << 2; conv |= (dcost < opt.absdcost) << 3;
        conv |= (fabs(maxstep) == INFINITY) << 4; conv |= (int)is_nan_bits(maxstep) << 5;
        conv |= (maxstep < opt.dstep) << 6; conv |= (fails > opt.maxfails) << 7; conv |= (iter >= opt.maxiters) << 8;
        if (conv) break;
        evaluate(vcur, true);                                                  // :167-170
    }
    if (!(bestcost >= cost)) SGL_FOR_ST(q) vcur[q] = vbest[q];      // updatefrombest!  :173-176
    return iter;
}

// ---- one THREAD per variable: many variables of a few blocks each (the points of a bundle adjustment)
__global__ __launch_bounds__(64) void singles_lm_kernel(const SinglesGroup* __restrict__ groups, const int64_t* __restrict__ selvar, int64_t nsel,
                                                        const int64_t* __restrict__ cptr, const int32_t* __restrict__ cgroup, const uint32_t* __restrict__ cidx,
                                                        const int32_t* __restrict__ cslot, const int32_t* __restrict__ vkind, const int32_t* __restrict__ vdim,
                                                        const uint32_t* __restrict__ voffs, SinglesOpt opt, double* __restrict__ vars, int64_t* __restrict__ iters_out) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= nsel) return;
    const int64_t v = selvar[t];
    const int kind = vkind[v], dim = vdim[v], nd = var_dof(kind, dim), ns = var_storage(kind, dim);
    const uint32_t off = voffs[v];
    double vcur[MAXST];
    for (int q = 0; q < ns; ++q) vcur[q] = vars[off + q];
    SinglesWork<SGL_MAXD> w; double* const g = w.g; double* const H = w.H;
    auto evaluate = [&](const double* vloc, bool want_gh) {
        double cost = 0;
        if (want_gh) { for (int i = 0; i < SGL_MAXD; ++i) g[i] = 0; for (int i = 0; i < SGL_MAXD * SGL_MAXD; ++i) H[i] = 0; }
        for (int64_t e = cptr[t]; e < cptr[t + 1]; ++e) {
            const SinglesGroup G = groups[cgroup[e]];
            switch (G.kind) {
#define X(K) case K: singles_block<K, SGL_MAXD, false>(G, cidx[e], cslot[e], vars, vloc, want_gh, cost, g, H); break;
                NLLS_FOR_EACH_RES(X)
#undef X
            }
        }
        return cost;
    };
    const int iter = singles_iterate<SGL_MAXD, false>(kind, dim, nd, ns, opt, vcur, w, evaluate);
    for (int q = 0; q < ns; ++q) vars[off + q] = vcur[q];
    iters_out[t] = iter;
}

// ---- one WAVEFRONT per variable: a variable of many blocks (a camera), or one wider than the thread kernel's 6 dof.  Lane l evaluates entries l, l + 64, ... of the
// variable's list and keeps private sums of the cost, g and the lower triangle of H in that order, in registers; the 64 partial sums are added in the fixed order of
// wave_sum_dpp63 and the total is read back from lane 63 by every lane: the result depends on nothing but the variable's own list (bit-reproducible, whatever else the
// launch holds).  Every lane then runs singles_iterate on the identical sums -- no divergence, no broadcast of the trial point -- and lane 0 writes the variable.  No atomics.
// MAXD: the bucket of the variable's dof (6 or SGL_WAVE_MAXD); every per-lane array is indexed at compile time (no scratch memory).
NLLS_DEV double wave_total(double v) {
    v = wave_sum_dpp63(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
template <int MAXD>
__global__ __launch_bounds__(64) void singles_wave_kernel(const SinglesGroup* __restrict__ groups, const int64_t* __restrict__ selvar,
                                                          const int64_t* __restrict__ cptr, const int32_t* __restrict__ cgroup, const uint32_t* __restrict__ cidx,
                                                          const int32_t* __restrict__ cslot, const int32_t* __restrict__ vkind, const int32_t* __restrict__ vdim,
                                                          const uint32_t* __restrict__ voffs, SinglesOpt opt, double* __restrict__ vars, int64_t* __restrict__ iters_out) {
    constexpr bool WAVE = true;
    __shared__ SinglesWork<MAXD> w;                            // (one wavefront per workgroup)
    const int64_t t = blockIdx.x; const int lane = threadIdx.x;
    const int64_t v = selvar[t];
    const int kind = vkind[v], dim = vdim[v], nd = var_dof(kind, dim), ns = var_storage(kind, dim);
    const uint32_t off = voffs[v];
    const int64_t e0 = cptr[t], e1 = cptr[t + 1];
    double vcur[MAXST];
    SGL_FOR_ST(q) vcur[q] = vars[off + q];
    auto evaluate = [&](const double* vloc, bool want_gh) {
        double cost = 0, g[MAXD], H[MAXD * MAXD];              // this lane's sums (of H only i >= j is ever touched)
        if (want_gh) {
#pragma unroll
            for (int j = 0; j < MAXD; ++j) { g[j] = 0;
#pragma unroll
                for (int i = j; i < MAXD; ++i) H[i + MAXD * j] = 0; }
        }
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            const SinglesGroup G = groups[cgroup[e]];
            switch (G.kind) {
#define X(K) case K: singles_block<K, MAXD, true>(G, cidx[e], cslot[e], vars, vloc, want_gh, cost, g, H); break;
                NLLS_FOR_EACH_RES(X)
#undef X
            }
        }
        cost = wave_total(cost);
        if (want_gh) {
#pragma unroll
            for (int j = 0; j < MAXD; ++j) if (j < nd) {
                w.g[j] = wave_total(g[j]);
#pragma unroll
                for (int i = j; i < MAXD; ++i) if (i < nd) { const double h = wave_total(H[i + MAXD * j]); w.H[i + MAXD * j] = h; w.H[j + MAXD * i] = h; }
            }
        }
        return cost;
    };
    const int iter = singles_iterate<MAXD, true>(kind, dim, nd, ns, opt, vcur, w, evaluate);
    if (lane == 0) { SGL_FOR_ST(q) vars[off + q] = vcur[q]; iters_out[t] = iter; }
}
#undef SGL_FOR_ST

// ================================================================================================
// host-side enqueue
// ================================================================================================

template <int KIND>
static int launch_cost(nlls_ctx* c, const Group& G, const double* vars, int64_t& pbase, const PostSolveArgs* post, bool* taken) {
    if (G.ncost > 0) {
        const int cost_grid_max = c->sw.cost_grid_max;   // (A/B: workgroups of the cost sweep)
        int grid = (int)std::min<int64_t>((G.ncost + TPB - 1) / TPB, cost_grid_max);
        const bool shared = G.cost_list >= 0 && c->info.is_sparse;
        const double* data = shared ? G.lists[G.cost_list].data.p : G.data.p; const uint32_t* voff = shared ? G.lists[G.cost_list].voff.p : G.voff.p;
        // (matrix-free LM trial: the blocks in elimination order are what the loop's other two launches stream -- the cost sweep reads the same 24 bytes per block)
        if (c->mf_ok && c->sw.mf_on && G.mf_data.p && G.mf_voff.p) { data = G.mf_data.p; voff = G.mf_voff.p; }
        if (post && taken && !*taken) {      // the first launch of the sweep takes the statistics roles along
            hipLaunchKernelGGL((cost_kernel<KIND, true>), dim3(grid + post->np + post->np3 + post->np2), dim3(TPB), 0, c->stream, vars, data, voff, (const uint32_t*)nullptr, G.ncost, G.rk, c->partials.p + pbase, grid, *post);
            *taken = true;
        } else hipLaunchKernelGGL((cost_kernel<KIND, false>), dim3(grid), dim3(TPB), 0, c->stream, vars, data, voff, (const uint32_t*)nullptr, G.ncost, G.rk, c->partials.p + pbase, grid, PostSolveArgs{});
        pbase += grid;
    }
    return NLLS_OK;
}
template <int KIND>
static int launch_fixedcost(nlls_ctx* c, const Group& G, const double* vars, int64_t& pbase) {
    if (G.nfixedcost > 0) {
        int grid = (int)std::min<int64_t>((G.nfixedcost + TPB - 1) / TPB, 2048);
        hipLaunchKernelGGL((cost_kernel<KIND, false>), dim3(grid), dim3(TPB), 0, c->stream, vars, G.data.p, G.voff.p, G.fixedcost.p, G.nfixedcost, G.rk, c->partials.p + pbase, grid, PostSolveArgs{});
        pbase += grid;
    }
    return NLLS_OK;
}
static int dyn_n_of(const Group& G) { return G.res_kind == NLLS_RES_DYN_LINEAR ? G.ndata - 1 : G.res_kind == NLLS_COST_DYN_LINEAR ? G.ndata : G.nres; }
static int launch_dyn_cost(nlls_ctx* c, const Group& G, const double* vars, int64_t& pbase, bool fixed_only) {
    const int64_t nb = fixed_only ? G.nfixedcost : G.ncost;
    if (nb > 0) {
        hipLaunchKernelGGL(dyn_block_kernel, dim3((unsigned)nb), dim3(TPB), 0, c->stream, G.res_kind, dyn_n_of(G), G.ndata, vars, G.data.p, G.voff.p,
                           fixed_only ? G.fixedcost.p : (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0, (double*)nullptr, (double*)nullptr, c->partials.p + pbase, G.rk);
        pbase += nb;
    }
    return NLLS_OK;
}
int enqueue_dyn_gradhess(nlls_ctx* c, const Group& G, const double* vars, int64_t& pbase) {
    if (G.dense.n > 0) {
        hipLaunchKernelGGL(dyn_block_kernel, dim3((unsigned)G.dense.n), dim3(TPB), 0, c->stream, G.res_kind, dyn_n_of(G), G.ndata, vars, G.dense.data.p, G.dense.voff.p,
                           (const uint32_t*)nullptr, G.dense.brow.p, (int)c->info.ndof, c->A.p, c->b.p, c->partials.p + pbase, G.rk, (const uint32_t*)(c->info.is_sparse ? G.dense.aoff.p : nullptr));
        pbase += G.dense.n;
    }
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}
// cost blocks whose variables are all fixed: cost only (called from the gradient sweep as well)
int enqueue_fixedcost(nlls_ctx* c, const Group& G, const double* vars, int64_t& pbase) {
    if (is_dyn_kind(G.res_kind)) return launch_dyn_cost(c, G, vars, pbase, true);
    return dispatch_res(G.res_kind, [&](auto k) { return launch_fixedcost<k()>(c, G, vars, pbase); }, NLLS_OK);
}
// ---- closed forms against dual numbers (nlls_check_analytic) --------------------------------------------------------------------------------------
// Every block of a group evaluated twice -- BlockGH<KIND, true> (a residual kind's own `jac`, the adaptive kernel's closed-form derivatives) and
// BlockGH<KIND, false> (everything through Dual<N> / Dual2: src/autodiff.jl:81-93,164-165 as written) -- and the largest difference of each quantity,
// relative to the largest magnitude of that quantity in the block: out[0] J, [1] J'r, [2] cost, [3] rho', [4] rho'', [5] d rho / d kernel, [6] d2 rho / d kernel d(kernel, cost).
template <int KIND>
__global__ __launch_bounds__(TPB) void check_analytic_kernel(const double* __restrict__ vars, const double* __restrict__ data, const uint32_t* __restrict__ voff, int64_t n,
                                                             RobustSpec rk, int kernel_free, double* __restrict__ out) {
    using R = Res<KIND>; using BA = BlockGH<KIND, true>; using BD = BlockGH<KIND, false>;
    __shared__ double red[TPB / 64];
    double m[7] = {0, 0, 0, 0, 0, 0, 0};
    if constexpr (!is_cost_kind<KIND>) {
        for (int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x; e < n; e += (int64_t)gridDim.x * TPB) {
            double d[R::NDATA]; uint32_t vo[R::NDEPS];
#pragma unroll
            for (int q = 0; q < R::NDATA; ++q) d[q] = data[(size_t)e * R::NDATA + q];
#pragma unroll
            for (int q = 0; q < R::NDEPS; ++q) vo[q] = voff[(size_t)e * R::NDEPS + q];
            BA a; a.compute(vars, vo, d, rk, kernel_free != 0);
            BD b; b.compute(vars, vo, d, rk, kernel_free != 0);
            auto upd = [](double& mx, double diff, double scale) { const double r = fabs(diff) / fmax(scale, 1e-300); if (!(r <= mx)) mx = r; };
            double sj = 0, sg = 0;
            for (int q = 0; q < BA::M; ++q) for (int j = 0; j < BA::NP; ++j) sj = fmax(sj, fabs(b.J[q][j]));
            for (int j = 0; j < BA::NP; ++j) sg = fmax(sg, fabs(b.g[j]));
            for (int q = 0; q < BA::M; ++q) for (int j = 0; j < BA::NP; ++j) upd(m[0], a.J[q][j] - b.J[q][j], sj);
            for (int j = 0; j < BA::NP; ++j) upd(m[1], a.g[j] - b.g[j], sg);
            upd(m[2], a.cost - b.cost, fabs(b.cost)); upd(m[3], a.dc - b.dc, fabs(b.dc)); upd(m[4], a.d2c - b.d2c, fmax(fabs(b.d2c), fabs(b.dc)));
            if constexpr (R::ADAPT) if (kernel_free) {
                double s1 = 0, s2 = 0;
                for (int i = 0; i < 3; ++i) { s1 = fmax(s1, fabs(b.dck[i])); for (int j = 0; j < 4; ++j) s2 = fmax(s2, fabs(b.d2ck[i][j])); }
                for (int i = 0; i < 3; ++i) { upd(m[5], a.dck[i] - b.dck[i], s1); for (int j = 0; j < 4; ++j) upd(m[6], a.d2ck[i][j] - b.d2ck[i][j], s2); }
            }
        }
    }
    for (int q = 0; q < 7; ++q) { const double t = block_max(m[q], red); if (threadIdx.x == 0) out[(size_t)blockIdx.x * 8 + q] = t; __syncthreads(); }
}
int enqueue_check_analytic(nlls_ctx* c, double* d_out /* [nblocks_total][8] */, int64_t* nblocks_out) {
    const double* vars = vars_ptr(c, NLLS_VARS_CURRENT); int64_t base = 0;
    for (const Group& G : c->groups) {
        if (is_dyn_kind(G.res_kind) || G.ncost == 0) continue;
        const int grid = (int)std::min<int64_t>((G.ncost + TPB - 1) / TPB, 256);
        if (d_out) dispatch_res(G.res_kind, [&](auto k) { hipLaunchKernelGGL(check_analytic_kernel<k()>, dim3(grid), dim3(TPB), 0, c->stream, vars, G.data.p, G.voff.p, G.ncost, G.rk, 1, d_out + base * 8); });
        base += grid;
    }
    if (nblocks_out) *nblocks_out = base;
    return hipGetLastError() == hipSuccess ? NLLS_OK : NLLS_ERR_HIP;
}

// ---- robustify / robustifydcost of one kernel at many costs (nlls_robustify): the two functions every kernel above calls ----------------------------------------------
__global__ __launch_bounds__(TPB) void robustify_kernel(RobustSpec rk, int64_t n, const double* __restrict__ cost, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const double c = cost[i]; double rho, d1, d2;
        robustifydcost_fixed(rk, c, rho, d1, d2);
        out[4 * i] = robustify_fixed(rk, c); out[4 * i + 1] = rho; out[4 * i + 2] = d1; out[4 * i + 3] = d2;
    }
}
int enqueue_robustify(nlls_ctx* c, const RobustSpec& rk, int64_t n, const double* d_cost, double* d_out) {
    if (n <= 0) return NLLS_OK;
    const int grid = (int)std::min<int64_t>((n + TPB - 1) / TPB, 1024);
    hipLaunchKernelGGL(robustify_kernel, dim3(grid), dim3(TPB), 0, c->stream, rk, n, d_cost, d_out);
    return hipGetLastError() == hipSuccess ? NLLS_OK : NLLS_ERR_HIP;
}

int enqueue_reduce_partials(nlls_ctx* c, int64_t n) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(TPB), 0, c->stream, c->partials.p, n, c->scalars.p);
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}

// pofs / count: an LM trial leaves the partials un-reduced at partials + pofs (count of them in *count) for enqueue_trial_finish
int enqueue_sweep_cost(nlls_ctx* c, int which, int64_t pofs, int64_t* count, const PostSolveArgs* post, bool* post_taken) {
    const double* vars = vars_ptr(c, which); int64_t pbase = pofs;
    for (const Group& G : c->groups) {
        if (is_dyn_kind(G.res_kind)) { launch_dyn_cost(c, G, vars, pbase, false); continue; }
        dispatch_res(G.res_kind, [&](auto k) { launch_cost<k()>(c, G, vars, pbase, post, post_taken); });
    }
    if (count) *count = pbase - pofs;
    else hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(TPB), 0, c->stream, c->partials.p + pofs, pbase - pofs, c->scalars.p);
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}

int enqueue_retract(nlls_ctx* c, int to, int from) {
    const int64_t nvar = c->info.nvar; if (nvar == 0) return NLLS_OK;
    hipLaunchKernelGGL(retract_kernel, dim3((unsigned)((nvar + 255) / 256)), dim3(256), 0, c->stream, c->d_var_kind.p, c->d_var_dim.p, c->d_var_off.p,
                       c->d_var_boff.p, nvar, vars_ptr(c, from), c->x.p, vars_ptr(c, to));
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}
int enqueue_step_stats(nlls_ctx* c) {
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((c->info.ndof + TPB - 1) / TPB, RED_BLOCKS));
    hipLaunchKernelGGL(step_stats_partial_kernel, dim3(nb), dim3(TPB), 0, c->stream, c->x.p, c->info.ndof, c->partials.p);
    hipLaunchKernelGGL(step_stats_finish_kernel, dim3(1), dim3(TPB), 0, c->stream, c->partials.p, nb, c->scalars.p);
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}
int enqueue_max_abs_diag(nlls_ctx* c) {
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((c->info.nblocks + TPB - 1) / TPB, RED_BLOCKS));
    hipLaunchKernelGGL(max_abs_diag_partial_kernel, dim3(nb), dim3(TPB), 0, c->stream, c->A.p, c->d_diag_off.p, c->d_blocksizes.p,
                       c->nranks > 1 ? c->d_row_mask.p : (const uint8_t*)nullptr, c->info.nblocks, c->info.is_sparse ? (int64_t)0 : c->info.ndof, c->partials.p);
    hipLaunchKernelGGL(max_finish_kernel, dim3(1), dim3(TPB), 0, c->stream, c->partials.p, nb, c->scalars.p, 3);
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}

// optimizesingles!: the launch.  The caller has validated the lists (nlls_optimize_singles).
// optimizesingles! under sharding: the storage of the listed variables, between the variable set and a dense buffer of the same layout (the ranks' results are
// gathered by a sum over buffers that are zero where another rank did the work)
__global__ void copy_var_storage_kernel(const int64_t* __restrict__ sel, int64_t nsel, const uint32_t* __restrict__ var_off, const double* __restrict__ src, double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i >= nsel) return;
    const int64_t v = sel[i];
    for (uint32_t q = var_off[v]; q < var_off[v + 1]; ++q) dst[q] = src[q];
}
__global__ void iters_to_double_kernel(const int64_t* __restrict__ it, const int64_t* __restrict__ pos, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[pos[i]] = (double)it[i];
}
int enqueue_copy_var_storage(nlls_ctx* c, const int64_t* d_sel, int64_t nsel, const double* src, double* dst) {
    if (nsel > 0) hipLaunchKernelGGL(copy_var_storage_kernel, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, c->stream, d_sel, nsel, c->d_var_off.p, src, dst);
    return hipGetLastError() == hipSuccess ? NLLS_OK : NLLS_ERR_HIP;
}
int enqueue_iters_to_double(nlls_ctx* c, const int64_t* d_it, const int64_t* d_pos, int64_t n, double* d_out) {
    if (n > 0) hipLaunchKernelGGL(iters_to_double_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_it, d_pos, n, d_out);
    return hipGetLastError() == hipSuccess ? NLLS_OK : NLLS_ERR_HIP;
}
// The listed variables come in three runs: [0, nthread) one per thread, then nwave6 of at most 6 dof and nwave12 of up to SGL_WAVE_MAXD dof, one per wavefront.  The
// variables of one call are independent, so the launches commute.
int enqueue_optimize_singles(nlls_ctx* c, int64_t nthread, int64_t nwave6, int64_t nwave12, const int64_t* d_selvar, const int64_t* d_cptr, const int32_t* d_cgroup, const uint32_t* d_cidx,
                             const int32_t* d_cslot, const void* d_groups, int iterator, int maxiters, int maxfails, double reldcost, double absdcost, double dstep, int64_t* d_iters) {
    SinglesOpt o{maxiters, maxfails, reldcost, absdcost, dstep, iterator};
    if (nthread > 0)
        hipLaunchKernelGGL(singles_lm_kernel, dim3((unsigned)((nthread + 63) / 64)), dim3(64), 0, c->stream, (const SinglesGroup*)d_groups, d_selvar, nthread, d_cptr, d_cgroup, d_cidx, d_cslot,
                           c->d_var_kind.p, c->d_var_dim.p, c->d_var_off.p, o, vars_ptr(c, NLLS_VARS_CURRENT), d_iters);
    int64_t first = nthread;                                   // (cptr holds absolute entry numbers: a run starts at its own slice of the three per-variable arrays)
    if (nwave6 > 0)
        hipLaunchKernelGGL(singles_wave_kernel<SGL_MAXD>, dim3((unsigned)nwave6), dim3(64), 0, c->stream, (const SinglesGroup*)d_groups, d_selvar + first, d_cptr + first, d_cgroup, d_cidx, d_cslot,
                           c->d_var_kind.p, c->d_var_dim.p, c->d_var_off.p, o, vars_ptr(c, NLLS_VARS_CURRENT), d_iters + first);
    first += nwave6;
    if (nwave12 > 0)
        hipLaunchKernelGGL(singles_wave_kernel<SGL_WAVE_MAXD>, dim3((unsigned)nwave12), dim3(64), 0, c->stream, (const SinglesGroup*)d_groups, d_selvar + first, d_cptr + first, d_cgroup, d_cidx, d_cslot,
                           c->d_var_kind.p, c->d_var_dim.p, c->d_var_off.p, o, vars_ptr(c, NLLS_VARS_CURRENT), d_iters + first);
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}
size_t singles_group_size() { return sizeof(SinglesGroup); }
void singles_group_fill(void* dst, const Group& G) { SinglesGroup g{G.res_kind, G.data.p, G.voff.p, G.rk}; memcpy(dst, &g, sizeof(g)); }

}  // namespace nlls
