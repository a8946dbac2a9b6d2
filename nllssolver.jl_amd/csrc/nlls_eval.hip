// nlls_eval.hip -- the cost blocks evaluated with their per-block values kept, and the adaptive kernel's Expectation-Maximization step (gfx950).
//
//   computeresidual(residual, vars...)                       src/NLLSsolver.jl:16
//   cost(residual, vars) = r'r, robustify, robustifydcost    src/residual.jl:49-55, src/robust.jl, src/robustadaptive.jl:25-33
//   optimize(kernel::ContaminatedGaussian, squarederrors)    src/robustadaptive.jl:48-73 (the EM callback of test/adaptivecost.jl:15-25)
//
// Built like nlls_cost.hip, WITHOUT -fno-honor-nans / -fno-signed-zeros: exp() overflowing to Inf for a far outlier must give the weight 1 / (1 + Inf) = 0 exactly, and
// a NaN residual must come out as NaN.  Reads the blocks in the caller's upload order (Group::data / voff), never the entry lists or the elimination order of the sweeps.
#include <algorithm>

#include "nlls_wave.hpp"

namespace nlls {

// ================================================================================================
// per-block values
// ================================================================================================
// One lane per block.  Any of the four outputs may be null (wave-uniform branches).  sel_voff != SEL_ALL: the EM step's evaluation -- sq_out[i] = r'r for the blocks whose
// slot 0 is stored at sel_voff and EM_SKIP for the others, and the workgroup leaves (sum of r'r, number of blocks) over the selected ones in part[2 bid], part[2 bid + 1].
constexpr uint32_t SEL_ALL = 0xFFFFFFFFu;
constexpr double EM_SKIP = -1.0;                               // (r'r is >= 0 or NaN: never this)
template <int KIND>
__global__ __launch_bounds__(TPB) void eval_blocks_kernel(const double* __restrict__ vars, const double* __restrict__ data, const uint32_t* __restrict__ voff, int64_t n,
                                                          RobustSpec rk, double* __restrict__ r_out, double* __restrict__ sq_out, double* __restrict__ rho_out,
                                                          double* __restrict__ w_out, uint32_t sel_voff, double* __restrict__ part) {
    using R = Res<KIND>; using I = ResInfo<KIND>;
    __shared__ double red[TPB / 64];
    double acc = 0, cnt = 0;
    if constexpr (!is_cost_kind<KIND>) {
        for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
            double d[R::NDATA > 0 ? R::NDATA : 1]; uint32_t vo[R::NDEPS];
#pragma unroll
            for (int q = 0; q < R::NDATA; ++q) d[q] = data[i * R::NDATA + q];
#pragma unroll
            for (int q = 0; q < R::NDEPS; ++q) vo[q] = voff[i * R::NDEPS + q];
            double sv[I::NS > 0 ? I::NS : 1][MAXST];
            [&]<int... S>(std::integer_sequence<int, S...>) {
                (var_load<R::SK[S + R::ADAPT], R::SD[S + R::ADAPT], double>(vars + vo[S + R::ADAPT], -1, sv[S]), ...);
            }(std::make_integer_sequence<int, I::NS>{});
            double r[R::M]; R::template eval<double>(d, sv, r);
            double s = 0;                                      // (the sum block_cost takes: the same bits as the cost sweep's r'r)
#pragma unroll
            for (int m = 0; m < R::M; ++m) s += r[m] * r[m];
            if (sel_voff != SEL_ALL) {
                const bool mine = vo[0] == sel_voff;
                sq_out[i] = mine ? s : EM_SKIP;
                if (mine) { acc += s; cnt += 1.0; }
                continue;
            }
            if (r_out) {
#pragma unroll
                for (int m = 0; m < R::M; ++m) r_out[i * R::M + m] = r[m];
            }
            if (sq_out) sq_out[i] = s;
            if (rho_out) { if constexpr (R::ADAPT) rho_out[i] = cg_robustify(vars + vo[0], s); else rho_out[i] = robustify_fixed(rk, s); }
            if (w_out) {
                double rho, d1, d2;
                if constexpr (R::ADAPT) cg_robustifydcost(vars + vo[0], s, rho, d1, d2); else robustifydcost_fixed(rk, s, rho, d1, d2);
                w_out[i] = d1;
            }
        }
    }
    if (part) {                                                // (uniform over the launch)
        const double ta = block_sum(acc, red);
        const double tc = block_sum(cnt, red);
        if (threadIdx.x == 0) { part[2 * blockIdx.x] = ta; part[2 * blockIdx.x + 1] = tc; }
    }
}

// The dynamic-size residual kinds (src/autodiff.jl:96-121): one workgroup per block, the sums taken as dyn_block_kernel (nlls_cost.hip) takes them.
//   NLLS_RES_DYN_LINEAR  X'w - y (nres 1)     NLLS_RES_DYN_NORM  w (nres n)     NLLS_RES_DYN_LINEARSQ  X w - y (nres n <= 512)
__global__ __launch_bounds__(TPB) void eval_dyn_kernel(int kind, int n, int ndata, const double* __restrict__ vars, const double* __restrict__ data, const uint32_t* __restrict__ voff,
                                                       RobustSpec rk, double* __restrict__ r_out, double* __restrict__ sq_out, double* __restrict__ rho_out, double* __restrict__ w_out) {
    __shared__ double red[TPB / 64]; __shared__ double rs[512];
    const int64_t k = blockIdx.x;
    const double* w = vars + voff[k]; const double* dd = data + k * (int64_t)ndata;
    double acc = 0;
    if (kind == NLLS_RES_DYN_LINEAR) {
        for (int i = threadIdx.x; i < n; i += TPB) acc += dd[1 + i] * w[i];
    } else if (kind == NLLS_RES_DYN_LINEARSQ) {
        const double* X = dd + n;
        for (int i = threadIdx.x; i < n; i += TPB) { double t = -dd[i]; for (int j = 0; j < n; ++j) t = fma(X[i + (size_t)n * j], w[j], t); rs[i] = t; if (r_out) r_out[k * (int64_t)n + i] = t; }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += TPB) acc += rs[i] * rs[i];
    } else {
        for (int i = threadIdx.x; i < n; i += TPB) { const double t = w[i]; acc += t * t; if (r_out) r_out[k * (int64_t)n + i] = t; }
    }
    const double total = block_sum(acc, red);                  // (valid in thread 0)
    if (threadIdx.x != 0) return;
    double s = total;
    if (kind == NLLS_RES_DYN_LINEAR) { const double r = total - dd[0]; if (r_out) r_out[k] = r; s = r * r; }
    if (sq_out) sq_out[k] = s;
    if (rho_out) rho_out[k] = robustify_fixed(rk, s);
    if (w_out) { double rho, d1, d2; robustifydcost_fixed(rk, s, rho, d1, d2); w_out[k] = d1; }
}

// ================================================================================================
// Expectation-Maximization of the ContaminatedGaussian kernel   src/robustadaptive.jl:48-73
// ================================================================================================
// The state of one call, in device memory: [0..2] the kernel's storage (1/sigma1, 1/sigma2, w), [3..5] oldparams, [6] sum(squarederrors), [7] length(squarederrors),
// [8] passes made, [9] done (isapprox held: the passes still enqueued return at once).
constexpr int EM_K = 0, EM_OLD = 3, EM_TOTAL = 6, EM_COUNT = 7, EM_ITERS = 8, EM_DONE = 9, EM_STATE = 16;
constexpr int EM_GRID_MAX = 512;                               // workgroups of a pass (and of the evaluation, per group)

// totalsquarederror, the number of blocks, and params(kernel) of the storage the set holds: one workgroup, the partials in a fixed order
__global__ __launch_bounds__(TPB) void em_init_kernel(const double* __restrict__ part, int npart, const double* __restrict__ kernel, double* __restrict__ state) {
    __shared__ double red[TPB / 64];
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < npart; i += TPB) { a += part[2 * i]; b += part[2 * i + 1]; }
    const double total = block_sum(a, red);
    const double count = block_sum(b, red);
    if (threadIdx.x == 0) {
        const double k0 = kernel[0], k1 = kernel[1], k2 = kernel[2];
        state[EM_K] = k0; state[EM_K + 1] = k1; state[EM_K + 2] = k2;
        state[EM_OLD] = 1.0 / k0; state[EM_OLD + 1] = 1.0 / k1; state[EM_OLD + 2] = k2;
        state[EM_TOTAL] = total; state[EM_COUNT] = count; state[EM_ITERS] = 0.0; state[EM_DONE] = 0.0;
    }
}
// The expectation step and the running totals of the maximization step (:53-63): every lane adds its entries in ascending index order, the workgroup's 256 sums are
// added in the fixed tree of block_sum, and the workgroup leaves (sum of w err, sum of w).  No atomics.
__global__ __launch_bounds__(TPB) void em_pass_kernel(const double* __restrict__ err, int64_t n, const double* __restrict__ state, double* __restrict__ part) {
    __shared__ double red[TPB / 64];
    if (state[EM_DONE] != 0.0) return;                         // (every lane reads the same word)
    const double is1 = state[EM_K], is2 = state[EM_K + 1], w = state[EM_K + 2];
    const double wratio = ((1.0 - w) * is2) / (is1 * w);
    const double h = -(0.5 * (is2 * is2 - is1 * is1));         // -kernel.halfs2sqminuss1sq
    double a = 0, b = 0;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const double e = err[i];
        if (e == EM_SKIP) continue;
        const double l = 1.0 / (1.0 + wratio * exp(h * e));    // exp -> Inf for a far outlier: the weight is exactly 0
        a += l * e; b += l;
    }
    const double ta = block_sum(a, red);
    const double tb = block_sum(b, red);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = ta; part[2 * blockIdx.x + 1] = tb; }
}
// The end of the maximization step (:65-70): the new parameters, the constructor's ordering (:12-19), isapprox(oldparams, newparams; rtol = 1e-6), and the storage
// written into the variable set.  One workgroup; one vector lane publishes.
__global__ __launch_bounds__(TPB) void em_finish_kernel(const double* __restrict__ part, int npart, double* __restrict__ state, double* __restrict__ kernel) {
    __shared__ double red[TPB / 64];
    if (state[EM_DONE] != 0.0) return;
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < npart; i += TPB) { a += part[2 * i]; b += part[2 * i + 1]; }
    const double sigma1 = block_sum(a, red);
    const double tw = block_sum(b, red);
    if (threadIdx.x != 0) return;
    const double total = state[EM_TOTAL], cnt = state[EM_COUNT];
    const double nw[3] = {sqrt(sigma1 / tw), sqrt((total - sigma1) / (cnt - tw)), tw / cnt};
    const double od[3] = {state[EM_OLD], state[EM_OLD + 1], state[EM_OLD + 2]};
    double k0 = 1.0 / nw[0], k1 = 1.0 / nw[1];
    if (!(k0 >= k1)) { const double t = k0; k0 = k1; k1 = t; }  // narrowest Gaussian first
    double dd = 0, no = 0, nn = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) { const double df = od[q] - nw[q]; dd += df * df; no += od[q] * od[q]; nn += nw[q] * nw[q]; }
    const bool same = sqrt(dd) <= 1e-6 * fmax(sqrt(no), sqrt(nn));   // (false for NaN, as in the reference: the passes go on)
    state[EM_K] = k0; state[EM_K + 1] = k1; state[EM_K + 2] = nw[2];
    state[EM_OLD] = nw[0]; state[EM_OLD + 1] = nw[1]; state[EM_OLD + 2] = nw[2];
    state[EM_ITERS] += 1.0;
    kernel[0] = k0; kernel[1] = k1; kernel[2] = nw[2];
    state[EM_DONE] = same ? 1.0 : 0.0;
}

// ================================================================================================
// host-side enqueue
// ================================================================================================
int eval_nres(const Group& G) { return G.res_kind == NLLS_RES_DYN_LINEAR ? 1 : G.nres; }
static int eval_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + TPB - 1) / TPB, 2048)); }

template <int KIND>
static void launch_eval(nlls_ctx* c, const Group& G, const double* vars, double* d_r, double* d_sq, double* d_rho, double* d_w, uint32_t sel, double* part, int grid) {
    hipLaunchKernelGGL(eval_blocks_kernel<KIND>, dim3(grid), dim3(TPB), 0, c->stream, vars, G.data.p, G.voff.p, G.ncost, G.rk, d_r, d_sq, d_rho, d_w, sel, part);
}
// the blocks of one group at vars[which]; the outputs are device pointers (null: not wanted)
int enqueue_eval_blocks(nlls_ctx* c, const Group& G, int which, double* d_r, double* d_sq, double* d_rho, double* d_w) {
    if (G.ncost == 0) return NLLS_OK;
    const double* vars = vars_ptr(c, which);
    if (is_dyn_kind(G.res_kind)) {
        const int n = G.res_kind == NLLS_RES_DYN_LINEAR ? G.ndata - 1 : G.nres;
        hipLaunchKernelGGL(eval_dyn_kernel, dim3((unsigned)G.ncost), dim3(TPB), 0, c->stream, G.res_kind, n, G.ndata, vars, G.data.p, G.voff.p, G.rk, d_r, d_sq, d_rho, d_w);
    } else dispatch_res(G.res_kind, [&](auto k) { launch_eval<k()>(c, G, vars, d_r, d_sq, d_rho, d_w, SEL_ALL, nullptr, eval_grid(G.ncost)); });
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}

// optimize(kernel, squarederrors, maxiters) for the kernel stored at kvoff of vars[which]: the evaluation of the adaptive groups, then every pass, enqueued back to
// back.  Leaves the call's state in c->em_state (EM_STATE doubles); the caller copies it home and synchronises.
int enqueue_adaptive_em(nlls_ctx* c, int which, uint32_t kvoff, int maxiters) {
    int64_t nerr = 0, npart = 0;
    for (const Group& G : c->groups) if (G.adaptive && G.ncost > 0) { nerr += G.ncost; npart += std::min(eval_grid(G.ncost), EM_GRID_MAX); }
    const int64_t need_part = 2 * std::max<int64_t>(npart, EM_GRID_MAX);
    if (c->em_err.n < (size_t)nerr) HIPCHK(c->em_err.alloc((size_t)nerr));
    if (c->em_part.n < (size_t)need_part) HIPCHK(c->em_part.alloc((size_t)need_part));
    if (c->em_state.n < (size_t)EM_STATE) HIPCHK(c->em_state.alloc(EM_STATE));
    double* vars = vars_ptr(c, which);
    int64_t ebase = 0, pbase = 0;
    for (const Group& G : c->groups) {
        if (!G.adaptive || G.ncost == 0) continue;
        const int grid = std::min(eval_grid(G.ncost), EM_GRID_MAX);
        dispatch_res(G.res_kind, [&](auto k) { launch_eval<k()>(c, G, vars, nullptr, c->em_err.p + ebase, nullptr, nullptr, kvoff, c->em_part.p + 2 * pbase, grid); });
        ebase += G.ncost; pbase += grid;
    }
    hipLaunchKernelGGL(em_init_kernel, dim3(1), dim3(TPB), 0, c->stream, c->em_part.p, (int)npart, vars + kvoff, c->em_state.p);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((nerr + TPB - 1) / TPB, EM_GRID_MAX));
    for (int it = 0; it < maxiters; ++it) {
        hipLaunchKernelGGL(em_pass_kernel, dim3(grid), dim3(TPB), 0, c->stream, c->em_err.p, nerr, c->em_state.p, c->em_part.p);
        hipLaunchKernelGGL(em_finish_kernel, dim3(1), dim3(TPB), 0, c->stream, c->em_part.p, grid, c->em_state.p, vars + kvoff);
    }
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}

}  // namespace nlls
