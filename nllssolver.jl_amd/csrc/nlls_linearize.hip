// nlls_linearize.hip -- the linearisation of single cost blocks handed out as it is, before any sum: residual and Jacobian, cost, gradient and Hessian per block (gfx950).
//
//   computeresjac(varflags = all free, residual, vars...)        src/autodiff.jl:78-93, src/NLLSsolver.jl:16
//   computecostgradhess / computerescostgradhess, all free       src/residual.jl:57-111, src/autodiff.jl:144-159
//
// Everything comes from the BlockGH<KIND> the sweeps use (nlls_kinds.hpp): the closed-form Jacobians of the pinhole kinds and the closed-form border of the adaptive
// kernel are what is exported.  Reads the blocks in the caller's upload order (Group::data / voff), never the entry lists or the matrix-free trial's arrays; writes only
// the call's own scratch.  Built like nlls_eval.hip, WITHOUT -fno-honor-nans / -fno-signed-zeros: a NaN residual comes out as NaN.
#include <algorithm>

#include "nlls_records.hpp"      // store_records: the records through a wavefront's LDS slab

namespace nlls {

// ================================================================================================
// per-block linearisation
// ================================================================================================
// sizes of a kind's records: J is M x NJ (column-major), g has P entries, H is P x P -- adaptive kinds: the kernel's three entries first (src/residual.jl:103-107)
template <int KIND> struct LinSize {
    static constexpr int M = Res<KIND>::M, NJ = ResInfo<KIND>::NP, P = NJ + 3 * Res<KIND>::ADAPT;
};
template <int KIND>
NLLS_DEV double lin_g(const BlockGH<KIND>& B, int i) {
    if constexpr (Res<KIND>::ADAPT) return i < 3 ? B.Gk(i < 3 ? i : 0) : B.G(i < 3 ? 0 : i - 3);
    else return B.G(i);
}
template <int KIND>
NLLS_DEV double lin_h(const BlockGH<KIND>& B, int i, int j) {
    if constexpr (Res<KIND>::ADAPT) {
        if (i < 3 && j < 3) return B.Hkk(i, j);
        if (i < 3) return B.Hkv(i, j - 3);
        if (j < 3) return B.Hkv(j, i - 3);
        return B.H(i - 3, j - 3);
    } else return B.H(i, j);
}

// One lane per selected block: block index[i] - 1 (index null: block i), record i of every output.  Any output may be null (wave-uniform branches); r and J only for
// kinds with a residual.  r is Res<KIND>::eval<double> -- the bits of nlls_eval_blocks; the rest is BlockGH with every slot free, the adaptive kernel included.
template <int KIND>
__global__ __launch_bounds__(TPB) void linearize_blocks_kernel(const double* __restrict__ vars, const double* __restrict__ data, const uint32_t* __restrict__ voff,
                                                               const int64_t* __restrict__ index, int64_t n, RobustSpec rk, double* __restrict__ r_out, double* __restrict__ J_out,
                                                               double* __restrict__ cost_out, double* __restrict__ g_out, double* __restrict__ H_out) {
    using R = Res<KIND>; using I = ResInfo<KIND>; using S = LinSize<KIND>;
    __shared__ double slabs[(TPB / 64) * LIN_WAVE_SLAB];
    double* slab = slabs + (threadIdx.x >> 6) * LIN_WAVE_SLAB;
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t first = (int64_t)blockIdx.x * TPB + (threadIdx.x & ~63u); first < n; first += (int64_t)gridDim.x * TPB) {
        const int cnt = (int)(n - first < 64 ? n - first : 64);
        BlockGH<KIND> B; double r[R::M];
        if (lane < cnt) {
            const int64_t k = index ? index[first + lane] - 1 : first + lane;
            double d[R::NDATA > 0 ? R::NDATA : 1]; uint32_t vo[R::NDEPS];
#pragma unroll
            for (int q = 0; q < R::NDATA; ++q) d[q] = data[k * R::NDATA + q];
#pragma unroll
            for (int q = 0; q < R::NDEPS; ++q) vo[q] = voff[k * R::NDEPS + q];
            B.compute(vars, vo, d, rk, /*kernel_free=*/true);
            if constexpr (!is_cost_kind<KIND>) {
                if (r_out) {
                    // the payload and the variables once more, through pointers the compiler cannot tell from the ones above: eval<double> then shares no subexpression
                    // with BlockGH's Jacobian, is contracted into the same fused multiply-adds as in eval_blocks_kernel, and r carries the bits of nlls_eval_blocks
                    const double* vars_r = vars; const double* data_r = data;
                    asm volatile("" : "+s"(vars_r), "+s"(data_r));
                    double dr[R::NDATA > 0 ? R::NDATA : 1];
#pragma unroll
                    for (int q = 0; q < R::NDATA; ++q) dr[q] = data_r[k * R::NDATA + q];
                    double sv[I::NS > 0 ? I::NS : 1][MAXST];
                    [&]<int... Q>(std::integer_sequence<int, Q...>) {
                        (var_load<R::SK[Q + R::ADAPT], R::SD[Q + R::ADAPT], double>(vars_r + vo[Q + R::ADAPT], -1, sv[Q]), ...);
                    }(std::make_integer_sequence<int, I::NS>{});
                    R::template eval<double>(dr, sv, r);
                }
            }
        }
        if constexpr (!is_cost_kind<KIND>) {
            if (r_out) store_records<S::M>(r_out, first, cnt, slab, [&](auto q) { return r[q()]; });
            if (J_out) store_records<S::M * S::NJ>(J_out, first, cnt, slab, [&](auto q) { return B.J[q() % S::M][q() / S::M]; });
        }
        if (cost_out && lane < cnt) cost_out[first + lane] = B.cost;
        if (g_out) store_records<S::P>(g_out, first, cnt, slab, [&](auto q) { return lin_g<KIND>(B, q()); });
        if (H_out) store_records<S::P * S::P>(H_out, first, cnt, slab, [&](auto q) { return lin_h<KIND>(B, q() % S::P, q() / S::P); });
    }
}

// ================================================================================================
// host side
// ================================================================================================
bool lin_sizes(int kind, LinSizes& s) {
    return dispatch_res(kind, [&](auto k) { using S = LinSize<k()>; s.m = is_cost_kind<k()> ? 0 : S::M; s.nj = S::NJ; s.p = S::P;
                                            s.batch_r = lin_batch(S::M); s.batch_j = lin_batch(S::M * S::NJ); s.batch_g = lin_batch(S::P); s.batch_h = lin_batch(S::P * S::P); return true; }, false);
}
int lin_wave_slab() { return LIN_WAVE_SLAB; }

// n selected blocks of one group at vars[which]: d_index their 1-based blocks on the device (null: the first n); the outputs are device pointers (null: not wanted).
// The caller has checked the kind (lin_sizes).  Under NLLS_OPT_PHASE_EVENTS the launch sits between phase_ev[10] and [11] (nlls_get_phase_times [10]).
int enqueue_linearize(nlls_ctx* c, const Group& G, int which, int64_t n, const int64_t* d_index, double* d_r, double* d_J, double* d_cost, double* d_g, double* d_H) {
    if (n <= 0) return NLLS_OK;
    const double* vars = vars_ptr(c, which);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + TPB - 1) / TPB, 2048));
    const bool timed = c->phase_on && c->phase_ev.size() >= 12;
    const bool known = dispatch_res(G.res_kind, [&](auto k) {
        if (timed) (void)hipEventRecord(c->phase_ev[10], c->stream);
        hipLaunchKernelGGL(linearize_blocks_kernel<k()>, dim3(grid), dim3(TPB), 0, c->stream, vars, G.data.p, G.voff.p, d_index, n, G.rk, d_r, d_J, d_cost, d_g, d_H);
        if (timed) { (void)hipEventRecord(c->phase_ev[11], c->stream); c->lin_pending = true; }
        return true; }, false);
    if (!known) { c->err = "nlls_linearize: no kernel for this residual kind"; return NLLS_ERR_UNSUPPORTED; }
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}

}  // namespace nlls
