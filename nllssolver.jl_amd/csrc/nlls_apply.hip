// nlls_apply.hip -- matrix-free products with the linearisation: y = (H + lambda I) v, u = J v, y = J' u and the diagonal blocks of H + lambda I (gfx950).
//
//   hessian * x, g' H g of the iterators      src/linearsystem.jl:180-190, src/iterators.jl:47-115
//   fast_bAb                                  src/utils.jl:71-106
//   uniformscaling!                           src/BlockSparseMatrix.jl:83-99
//
// H = sum over blocks of P' H_blk P with the H_blk of nlls_eval_gradhess (BlockGH<KIND>, nlls_kinds.hpp), evaluated at the variable set of the call -- never read from
// A.data.  Two launches per chunk of vectors and no atomics: the block launch (one lane per cost block, caller's upload order, BlockGH::compute once per block) leaves
// one record per block and vector; the gather launch sums, per unfixed variable, the records of its incidences in ascending (group, block, slot) order (a row of more
// than APP_SEGMENT incidences: segment by segment, and a finishing launch adds the segments in order).  Reads only the
// context: Group::data / voff, the variables, and an index of its own built at the first call after an upload (nlls::ApplyIndex).
// Built like nlls_linearize.hip, WITHOUT -fno-honor-nans / -fno-signed-zeros: a NaN residual shows as NaN in the rows it touches.
#include <algorithm>

#include "nlls_records.hpp"

namespace nlls {

enum { APP_HESS = 0, APP_JAC = 1, APP_JACT = 2, APP_DIAG = 3, APP_OFFD = 4 };

// ================================================================================================
// block launch
// ================================================================================================
// A block's local unknowns: the kernel's three first (adaptive kinds), then the non-kernel slots in slot order -- the order of nlls_eval_gradhess.
template <int KIND> struct AppSize {
    using R = Res<KIND>; using I = ResInfo<KIND>;
    static constexpr int M = R::M, NJ = I::NP, KD = 3 * R::ADAPT, P = NJ + KD, ND = R::NDEPS;
    static constexpr int dof(int s) { return I::dof(s); }
    static constexpr int loff(int s) { return (R::ADAPT && s == 0) ? 0 : KD + I::joff(s); }            // first local unknown of slot s
    static constexpr int doff(int s) { int n = 0; for (int t = 0; t < s; ++t) n += dof(t) * dof(t); return n; }   // first entry of slot s's diagonal block in a record
    static constexpr int DD = doff(ND);
    static constexpr int dslot(int q) { int s = 0; while (s + 1 < ND && q >= doff(s + 1)) ++s; return s; }
    // the off-diagonal blocks of H_blk, one per slot pair s < t in the order (0, 1), (0, 2), .., (1, 2), ..: first entry of pair (s, t) in a record (a pair that does
    // not exist: the records' length), and the pair s * ND + t that entry q belongs to
    static constexpr int ooff(int s, int t) { int n = 0; for (int a = 0; a < ND; ++a) for (int b = a + 1; b < ND; ++b) { if (a == s && b == t) return n; n += dof(a) * dof(b); } return n; }
    static constexpr int OD = ooff(ND, ND);
    static constexpr int opair(int q) { int n = 0; for (int a = 0; a < ND; ++a) for (int b = a + 1; b < ND; ++b) { n += dof(a) * dof(b); if (q < n) return a * ND + b; } return 0; }
    static_assert(!R::ADAPT || I::dof(0) == 3, "the adaptive kernel is slot 0, three unknowns");
};
template <int KIND>
NLLS_DEV double app_h(const BlockGH<KIND>& B, int i, int j) {          // entry (i, j) of H_blk over the local unknowns
    if constexpr (Res<KIND>::ADAPT) {
        if (i < 3 && j < 3) return B.Hkk(i, j);
        if (i < 3) return B.Hkv(i, j - 3);
        if (j < 3) return B.Hkv(j, i - 3);
        return B.H(i - 3, j - 3);
    } else return B.H(i, j);
}
// y = H_blk x without forming H_blk: H(i, j) = sum_m Jw[m][i] J[m][j] + gw[i] g[j] (BlockGH::H), the kernel border g[i] d2ck[k][3] and d2ck[k][l] (Hkv, Hkk)
template <int KIND>
NLLS_DEV void app_hx(const BlockGH<KIND>& B, const double* x, double* y) {
    using S = AppSize<KIND>;
    if constexpr (is_cost_kind<KIND>) {
#pragma unroll
        for (int i = 0; i < S::P; ++i) { double s = 0;
#pragma unroll
            for (int j = 0; j < S::P; ++j) s += B.hc[i][j] * x[j];
            y[i] = s; }
    } else {
        double t[S::M], gx = 0, kx = 0;
#pragma unroll
        for (int m = 0; m < S::M; ++m) { double s = 0;
#pragma unroll
            for (int j = 0; j < S::NJ; ++j) s += B.J[m][j] * x[S::KD + j];
            t[m] = s; }
#pragma unroll
        for (int j = 0; j < S::NJ; ++j) gx += B.g[j] * x[S::KD + j];
        if constexpr (S::KD > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) kx += B.d2ck[k][3] * x[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) { double s = B.d2ck[k][3] * gx;
#pragma unroll
                for (int l = 0; l < 3; ++l) s += B.d2ck[k][l] * x[l];
                y[k] = s; }
        }
#pragma unroll
        for (int i = 0; i < S::NJ; ++i) { double s = B.gw[i] * gx;
#pragma unroll
            for (int m = 0; m < S::M; ++m) s += B.Jw[m][i] * t[m];
            if constexpr (S::KD > 0) s += B.g[i] * kx;
            y[S::KD + i] = s; }
    }
}

// One lane per cost block of a group, block i of the caller's upload order.  boff[i * ND + s]: where slot s's variable starts in b (DEST_NONE: fixed -- its entries of
// v count as 0 and nobody gathers its rows of the record).  Vector k: in + k * in_stride -> out + k * out_stride.
//   APP_HESS  in = v,  record i of out: P doubles, H_blk P' P v          APP_JAC   in = v,  out = u: M doubles per block, J P v
//   APP_JACT  in = u,  record i of out: P doubles, J' u (kernel rows 0)  APP_DIAG  one "vector": record i = the slots' diagonal blocks of H_blk, column-major each
//   APP_OFFD  one "vector": record i = for every slot pair s < t the block H_blk[slot s rows, slot t columns], column-major dof_s x dof_t (AppSize::ooff)
// The k loop is a run-time loop over one body: vector k of a call of many carries the bits of a call of its own.
template <int KIND, int MODE>
__global__ __launch_bounds__(TPB) void apply_blocks_kernel(const double* __restrict__ vars, const double* __restrict__ data, const uint32_t* __restrict__ voff,
                                                           const uint32_t* __restrict__ boff, int64_t n, RobustSpec rk, int nvec, const double* __restrict__ in, int64_t in_stride,
                                                           double* __restrict__ out, int64_t out_stride) {
    using R = Res<KIND>; using S = AppSize<KIND>;
    __shared__ double slabs[(TPB / 64) * LIN_WAVE_SLAB];
    double* slab = slabs + (threadIdx.x >> 6) * LIN_WAVE_SLAB;
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t first = (int64_t)blockIdx.x * TPB + (threadIdx.x & ~63u); first < n; first += (int64_t)gridDim.x * TPB) {
        const int cnt = (int)(n - first < 64 ? n - first : 64);
        const bool live = lane < cnt;
        BlockGH<KIND> B; uint32_t bo[S::ND];
#pragma unroll
        for (int q = 0; q < S::ND; ++q) bo[q] = DEST_NONE;
        if (live) {
            const int64_t k = first + lane;
            double d[R::NDATA > 0 ? R::NDATA : 1]; uint32_t vo[R::NDEPS];
#pragma unroll
            for (int q = 0; q < R::NDATA; ++q) d[q] = data[k * R::NDATA + q];
#pragma unroll
            for (int q = 0; q < R::NDEPS; ++q) { vo[q] = voff[k * R::NDEPS + q]; bo[q] = boff[k * R::NDEPS + q]; }
            B.compute(vars, vo, d, rk, /*kernel_free=*/true);
        }
        if constexpr (MODE == APP_DIAG) {
            store_records<S::DD>(out, first, cnt, slab, [&](auto q) {
                constexpr int s = S::dslot(q()), e = q() - S::doff(s), ds = S::dof(s);
                return app_h<KIND>(B, S::loff(s) + e % ds, S::loff(s) + e / ds); });
        } else if constexpr (MODE == APP_OFFD) {
            if constexpr (S::OD > 0)
                store_records<S::OD>(out, first, cnt, slab, [&](auto q) {
                    constexpr int pr = S::opair(q()), s = pr / S::ND, t = pr % S::ND, e = q() - S::ooff(s, t), ds = S::dof(s);
                    return app_h<KIND>(B, S::loff(s) + e % ds, S::loff(t) + e / ds); });
        } else {
            for (int k = 0; k < nvec; ++k) {
                const double* __restrict__ ik = in + (int64_t)k * in_stride; double* __restrict__ ok = out + (int64_t)k * out_stride;
                double x[S::P], y[MODE == APP_JAC ? S::M : S::P];
                if constexpr (MODE == APP_JACT) {
                    double u[S::M];
#pragma unroll
                    for (int m = 0; m < S::M; ++m) u[m] = live ? ik[(first + lane) * S::M + m] : 0.0;
#pragma unroll
                    for (int q = 0; q < S::KD; ++q) y[q] = 0.0;
#pragma unroll
                    for (int j = 0; j < S::NJ; ++j) { double s = 0;
#pragma unroll
                        for (int m = 0; m < S::M; ++m) s += B.J[m][j] * u[m];
                        y[S::KD + j] = s; }
                } else {
                    static_for<S::ND>([&](auto s) { constexpr int ds = S::dof(s()), lo = S::loff(s()); const uint32_t o = bo[s()];
#pragma unroll
                        for (int q = 0; q < ds; ++q) x[lo + q] = o != DEST_NONE ? ik[o + q] : 0.0; });
                    if constexpr (MODE == APP_JAC) {
#pragma unroll
                        for (int m = 0; m < S::M; ++m) { double s = 0;
#pragma unroll
                            for (int j = 0; j < S::NJ; ++j) s += B.J[m][j] * x[S::KD + j];
                            y[m] = s; }
                    } else app_hx<KIND>(B, x, y);
                }
                store_records<(MODE == APP_JAC ? S::M : S::P)>(ok, first, cnt, slab, [&](auto q) { return y[q()]; });
            }
        }
    }
}

// ================================================================================================
// gather launch
// ================================================================================================
// Output element e (an unknown of y; an entry of a diagonal block) belongs to block row erow[e], entry q = e - start[row] of it.  The row's incidences are
// offs[rowptr[row] .. rowptr[row + 1]): where the slot's entries start in one vector's records; only those in [lo, hi) count (one group's: nlls_jact_apply), read at
// rec[o - lo + q].  Summed in list order, then lambda * v[e] (v non-null) or lambda on the diagonal of the block (bsz non-null).
struct GatherArgs {
    const uint32_t* rowptr; const uint32_t* offs; const uint32_t* erow; const uint32_t* start; const int32_t* bsz; const LongItem* items; const BigRow* big;
    int64_t nelem, nitems, nbig; uint32_t wave_min, lo, hi; int diag;
    const double* rec; int64_t rec_stride; int nvec; double lambda; const double* v; double* y; int64_t y_stride; double* part; int part_w;
};
NLLS_DEV double gather_tail(const GatherArgs& a, int k, int64_t e, uint32_t q, int32_t d, double s) {
    if (a.diag) { if (q % (uint32_t)(d + 1) == 0) s += a.lambda; }
    else if (a.v) s += a.lambda * a.v[(int64_t)k * a.y_stride + e];
    return s;
}
// short rows (fewer than wave_min incidences): one lane per output element -- the lanes of a row read neighbouring doubles of the same records, several rows to a wavefront
__global__ __launch_bounds__(TPB) void apply_gather_short_kernel(GatherArgs a) {
    const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (e >= a.nelem) return;
    const uint32_t row = a.erow[e], p0 = a.rowptr[row], p1 = a.rowptr[row + 1];
    if (p1 - p0 >= a.wave_min) return;
    const uint32_t q = (uint32_t)(e - a.start[row]); const int32_t d = a.bsz[row];
    for (int k = 0; k < a.nvec; ++k) {
        const double* __restrict__ r = a.rec + (int64_t)k * a.rec_stride; double s = 0;
        for (uint32_t p = p0; p < p1; ++p) { const uint32_t o = a.offs[p]; if (o >= a.lo && o < a.hi) s += r[(o - a.lo) + q]; }
        a.y[(int64_t)k * a.y_stride + e] = gather_tail(a, k, e, q, d, s);
    }
}
// long rows: a wavefront per item -- a row of at most APP_SEGMENT incidences is one item and is written where it belongs; a longer one (the adaptive kernel's variable:
// every block of its group) is cut into segments of APP_SEGMENT, each leaves its sum in `part`, and apply_gather_finish_kernel adds the segments in order.  Lane l sums
// incidences l, l + 64, ... of the item in list order, then a fixed tree over the lanes.
__global__ __launch_bounds__(TPB) void apply_gather_long_kernel(GatherArgs a) {
    const int64_t w = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (w >= a.nitems) return;
    const int lane = (int)(threadIdx.x & 63);
    const LongItem it = a.items[w]; const uint32_t row = it.row;
    const int32_t d = a.bsz[row]; const uint32_t width = (uint32_t)(a.diag ? d * d : d); const int64_t e0 = a.start[row];
    for (int k = 0; k < a.nvec; ++k) {
        const double* __restrict__ r = a.rec + (int64_t)k * a.rec_stride;
        for (uint32_t q = 0; q < width; ++q) {
            double s = 0;
            for (uint32_t p = it.p0 + lane; p < it.p1; p += 64) { const uint32_t o = a.offs[p]; if (o >= a.lo && o < a.hi) s += r[(o - a.lo) + q]; }
            s = wave_sum(s);
            if (lane == 0) { if (it.slot == DEST_NONE) a.y[(int64_t)k * a.y_stride + e0 + q] = gather_tail(a, k, e0 + q, q, d, s);
                             else a.part[((int64_t)it.slot * a.nvec + k) * a.part_w + q] = s; }
        }
    }
}
// one lane per (cut row, entry): the row's segments in order
__global__ __launch_bounds__(TPB) void apply_gather_finish_kernel(GatherArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t b = t / a.part_w; const uint32_t q = (uint32_t)(t - b * a.part_w);
    if (b >= a.nbig) return;
    const BigRow br = a.big[b]; const int32_t d = a.bsz[br.row];
    if (q >= (uint32_t)(a.diag ? d * d : d)) return;
    const int64_t e = (int64_t)a.start[br.row] + q;
    for (int k = 0; k < a.nvec; ++k) { double s = 0;
        for (uint32_t i = 0; i < br.nslots; ++i) s += a.part[((int64_t)(br.slot0 + i) * a.nvec + k) * a.part_w + q];
        a.y[(int64_t)k * a.y_stride + e] = gather_tail(a, k, e, q, d, s); }
}

// ================================================================================================
// host side
// ================================================================================================
namespace {
struct AppDims { int nd = 0, m = 0, p = 0, dd = 0; bool cost = false; int loff[MAX_SLOTS] = {}, doff[MAX_SLOTS] = {}; };
bool app_dims(int kind, AppDims& a) {
    if (is_dyn_kind(kind)) return false;
    return dispatch_res(kind, [&](auto k) { using S = AppSize<k()>; a.nd = S::ND; a.m = S::M; a.p = S::P; a.dd = S::DD; a.cost = is_cost_kind<k()>;
                                            for (int s = 0; s < S::ND; ++s) { a.loff[s] = S::loff(s); a.doff[s] = S::doff(s); } return true; }, false);
}
constexpr uint64_t APP_MAX_OFF = 0xFFFFFFF0ull;

// The index of the products, built once per upload: per (block, slot) of every group where its variable sits in b, and per unfixed variable the CSR list of its
// incidences in ascending (group, block, slot) order.  Group::voff holds storage offsets; var_off maps them back to variables.
int apply_prepare(nlls_ctx* c) {
    ApplyIndex& X = c->app;
    if (X.ready) return NLLS_OK;
    const size_t nb = c->blocksizes.size(), ng = c->groups.size(), nvar = c->var_kind.size();
    X.boff.resize(ng); X.gbase_vec.assign(ng, -1); X.gbase_diag.assign(ng, -1);
    std::vector<std::vector<uint32_t>> hb(ng);       // the groups' incidence tables on the host: block + 1 (0: fixed)
    std::vector<AppDims> dims(ng);
    std::vector<uint32_t> cnt(nb + 1, 0);
    uint64_t rv = 0, rd = 0, ninc = 0;
    for (size_t g = 0; g < ng; ++g) { const Group& G = c->groups[g]; AppDims& D = dims[g];
        if (!app_dims(G.res_kind, D)) continue;
        X.gbase_vec[g] = (int64_t)rv; X.gbase_diag[g] = (int64_t)rd; rv += (uint64_t)G.ncost * D.p; rd += (uint64_t)G.ncost * D.dd;
        const size_t n = (size_t)G.ncost * D.nd; if (!n) continue;
        std::vector<uint32_t> hv(n), bo(n); hb[g].resize(n);
        HIPCHK(hipMemcpy(hv.data(), G.voff.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));       // (written once, by the upload)
        for (size_t i = 0; i < n; ++i) {
            const size_t var = (size_t)(std::upper_bound(c->var_off.begin(), c->var_off.begin() + nvar, hv[i]) - c->var_off.begin()) - 1;
            const uint64_t bi = c->blockindices[var];
            hb[g][i] = (uint32_t)bi; bo[i] = bi ? (uint32_t)c->boffsets[bi - 1] : DEST_NONE;
            if (bi) { ++cnt[bi]; ++ninc; } }
        HIPCHK(X.boff[g].upload(bo)); }
    if (rv > APP_MAX_OFF || rd > APP_MAX_OFF || ninc > APP_MAX_OFF) { c->err = "matrix-free products: the records of one vector exceed 32-bit offsets"; return NLLS_ERR_UNSUPPORTED; }
    X.rec_vec = (int64_t)rv; X.rec_diag = (int64_t)rd;
    X.h_rowptr.assign(nb + 1, 0);
    for (size_t b = 0; b < nb; ++b) X.h_rowptr[b + 1] = X.h_rowptr[b] + cnt[b + 1];
    std::vector<uint32_t> cur(X.h_rowptr.begin(), X.h_rowptr.end() - 1), ov(ninc), od(ninc);
    for (size_t g = 0; g < ng; ++g) { const AppDims& D = dims[g]; if (hb[g].empty()) continue;
        const int64_t nc = c->groups[g].ncost;
        for (int64_t k = 0; k < nc; ++k) for (int s = 0; s < D.nd; ++s) { const uint32_t bi = hb[g][(size_t)k * D.nd + s]; if (!bi) continue;
            const uint32_t at = cur[bi - 1]++;
            ov[at] = (uint32_t)(X.gbase_vec[g] + k * D.p + D.loff[s]); od[at] = (uint32_t)(X.gbase_diag[g] + k * D.dd + D.doff[s]); } }
    std::vector<uint32_t> ev((size_t)c->info.ndof), sv(nb), sd(nb); uint64_t nd2 = 0;
    for (size_t b = 0; b < nb; ++b) { sv[b] = (uint32_t)c->boffsets[b]; sd[b] = (uint32_t)nd2; const uint64_t d = (uint64_t)c->blocksizes[b];
        for (uint64_t q = 0; q < d; ++q) ev[(size_t)c->boffsets[b] + q] = (uint32_t)b;
        nd2 += d * d; }
    if (nd2 > APP_MAX_OFF) { c->err = "matrix-free products: the diagonal blocks exceed 32-bit offsets"; return NLLS_ERR_UNSUPPORTED; }
    std::vector<uint32_t> ed((size_t)nd2);
    for (size_t b = 0; b < nb; ++b) { const uint64_t d = (uint64_t)c->blocksizes[b]; for (uint64_t q = 0; q < d * d; ++q) ed[sd[b] + q] = (uint32_t)b; }
    X.nelem_diag = (int64_t)nd2;
    HIPCHK(X.rowptr.upload(X.h_rowptr)); HIPCHK(X.off_vec.upload(ov)); HIPCHK(X.off_diag.upload(od));
    HIPCHK(X.erow_vec.upload(ev)); HIPCHK(X.erow_diag.upload(ed)); HIPCHK(X.start_vec.upload(sv)); HIPCHK(X.start_diag.upload(sd));
    X.ready = true;
    return NLLS_OK;
}
}  // namespace
// The row-class rule, for the listed block rows (`blocks` null: all of them, in order): a row of `wave_min` incidences or more takes wavefronts -- one item per row, or
// per segment of APP_SEGMENT incidences of a longer row, whose segments' sums go to consecutive slots of `part`.  The products of this file and the class-restricted
// gathers of nlls_schur_apply.hip take their lists from here.
void classify_rows(const nlls_ctx* c, const uint32_t* blocks, size_t n, int64_t wave_min, RowClasses& out) {
    const ApplyIndex& X = c->app; out = RowClasses{};
    for (size_t i = 0; i < n; ++i) { const uint32_t b = blocks ? blocks[i] : (uint32_t)i; const uint32_t p0 = X.h_rowptr[b], p1 = X.h_rowptr[b + 1];
        if ((int64_t)(p1 - p0) < wave_min) { out.short_rows.push_back(b); continue; }
        out.long_rows.push_back(b);
        if (p1 - p0 <= APP_SEGMENT) { out.items.push_back(LongItem{b, p0, p1, DEST_NONE}); continue; }
        BigRow br{b, out.nslots, 0};
        for (uint32_t p = p0; p < p1; p += APP_SEGMENT) { out.items.push_back(LongItem{b, p, std::min(p + APP_SEGMENT, p1), out.nslots++}); ++br.nslots; }
        out.big.push_back(br); out.part_w_vec = std::max(out.part_w_vec, (int)c->blocksizes[b]); out.part_w_diag = std::max(out.part_w_diag, (int)c->blocksizes[b] * (int)c->blocksizes[b]); }
}
namespace {
// the rows that take wavefronts, under the threshold the context holds now
int apply_classify(nlls_ctx* c) {
    ApplyIndex& X = c->app;
    const int64_t wm = std::max<int64_t>(c->app_wave_min, 1);
    if (X.wave_min_built == wm) return NLLS_OK;
    RowClasses R; classify_rows(c, nullptr, X.h_rowptr.size() - 1, wm, R);
    HIPCHK(X.long_items.upload(R.items)); HIPCHK(X.big_rows.upload(R.big));
    X.nlong = (int64_t)R.long_rows.size(); X.nitems = (int64_t)R.items.size(); X.nbig = (int64_t)R.big.size(); X.nslots = R.nslots; X.part_w_vec = R.part_w_vec; X.part_w_diag = R.part_w_diag;
    X.wave_min_built = wm;
    return NLLS_OK;
}
int apply_scratch(nlls_ctx* c, int64_t per_vec, int nvec, int& chunk) {
    ApplyIndex& X = c->app;
    chunk = (int)std::clamp<int64_t>(per_vec > 0 ? c->app_scratch_cap / (8 * per_vec) : nvec, 1, nvec);
    const size_t need = (size_t)std::max<int64_t>(per_vec * chunk, 1);
    if (X.rec.n < need || !X.rec.p) { const hipError_t e = X.rec.alloc(need); if (e != hipSuccess) { X.rec.release(); (void)hipGetLastError(); return hip_fail(c, e, "matrix-free products: scratch for the records"); } }
    c->app_scratch = per_vec * chunk;
    return NLLS_OK;
}
template <int MODE>
int launch_blocks(nlls_ctx* c, size_t g, int which, int nvec, const double* in, int64_t in_stride, double* out, int64_t out_stride, const uint32_t* boff = nullptr) {      // boff: a table of the caller's (nlls_schur_apply.hip) in place of ApplyIndex::boff
    const Group& G = c->groups[g];
    if (G.ncost <= 0) return NLLS_OK;
    const double* vars = vars_ptr(c, which);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((G.ncost + TPB - 1) / TPB, 2048));
    const bool known = dispatch_res(G.res_kind, [&](auto k) {
        if constexpr (is_cost_kind<k()> && (MODE == APP_JAC || MODE == APP_JACT)) return false;
        else if constexpr (MODE == APP_OFFD && AppSize<k()>::OD == 0) return true;      // (a kind of one slot: no record, no launch)
        else { hipLaunchKernelGGL((apply_blocks_kernel<k(), MODE>), dim3(grid), dim3(TPB), 0, c->stream, vars, G.data.p, G.voff.p, boff ? boff : c->app.boff[g].p, G.ncost, G.rk, nvec, in, in_stride, out, out_stride);
               return true; } }, false);
    if (!known) { c->err = "matrix-free products: no kernel for this residual kind"; return NLLS_ERR_UNSUPPORTED; }
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}
int launch_gather(nlls_ctx* c, bool diag, uint32_t lo, uint32_t hi, int64_t rec_stride, int nvec, double lambda, const double* v, double* y) {
    ApplyIndex& X = c->app;
    GatherArgs a{};
    a.rowptr = X.rowptr.p; a.offs = diag ? X.off_diag.p : X.off_vec.p; a.erow = diag ? X.erow_diag.p : X.erow_vec.p; a.start = diag ? X.start_diag.p : X.start_vec.p;
    a.bsz = c->d_blocksizes.p; a.items = X.long_items.p; a.big = X.big_rows.p; a.nelem = diag ? X.nelem_diag : c->info.ndof; a.nitems = X.nitems; a.nbig = X.nbig;
    a.wave_min = (uint32_t)std::min<int64_t>(X.wave_min_built, 0xFFFFFFFFll); a.lo = lo; a.hi = hi; a.diag = diag ? 1 : 0;
    a.rec = X.rec.p; a.rec_stride = rec_stride; a.nvec = nvec; a.lambda = lambda; a.v = v; a.y = y; a.y_stride = a.nelem; a.part_w = diag ? X.part_w_diag : X.part_w_vec;
    if (X.nbig > 0) { const size_t need = (size_t)X.nslots * (size_t)nvec * (size_t)a.part_w;
        if (X.part.n < need || !X.part.p) { const hipError_t e = X.part.alloc(need); if (e != hipSuccess) { X.part.release(); (void)hipGetLastError(); return hip_fail(c, e, "matrix-free products: partial sums of the cut rows"); } } }
    a.part = X.part.p;
    if (a.nelem > 0) hipLaunchKernelGGL(apply_gather_short_kernel, dim3((unsigned)((a.nelem + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, a);
    if (a.nitems > 0) hipLaunchKernelGGL(apply_gather_long_kernel, dim3((unsigned)((a.nitems + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, c->stream, a);
    if (a.nbig > 0) hipLaunchKernelGGL(apply_gather_finish_kernel, dim3((unsigned)((a.nbig * a.part_w + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return NLLS_OK;
}
struct PhasePair {          // the call's launches between phase_ev[12] and [13] (nlls_get_phase_times [12], [13])
    nlls_ctx* c; bool on;
    explicit PhasePair(nlls_ctx* ctx) : c(ctx), on(ctx->phase_on && ctx->phase_ev.size() >= 14) { if (on) (void)hipEventRecord(c->phase_ev[12], c->stream); }
    void close(double bytes) { if (on) { (void)hipEventRecord(c->phase_ev[13], c->stream); c->app_pending = true; c->app_bytes = bytes; } }
};
}  // namespace

int64_t apply_diag_len(const nlls_ctx* c) { int64_t n = 0; for (int32_t d : c->blocksizes) n += (int64_t)d * d; return n; }

// what every product refuses, before anything is built or enqueued.  group < 0: all groups (H); need_residual: J of a non-squared cost kind does not exist
int apply_check(nlls_ctx* c, const char* name, int group, bool need_residual) {
    const std::string nm(name);
    if (c->nranks > 1) { c->err = nm + " under nlls_set_shard: a rank holds only its own cost blocks"; return NLLS_ERR_UNSUPPORTED; }
    if (group >= (int)c->groups.size()) { c->err = nm + ": bad cost group"; return NLLS_ERR_INVALID_ARG; }
    for (size_t g = 0; g < c->groups.size(); ++g) { if (group >= 0 && (size_t)group != g) continue;
        AppDims D;
        if (!app_dims(c->groups[g].res_kind, D)) { c->err = nm + ": a dynamic-size kind has no per-block Hessian"; return NLLS_ERR_UNSUPPORTED; }
        if (need_residual && D.cost) { c->err = nm + ": a non-squared cost kind has no residual"; return NLLS_ERR_UNSUPPORTED; } }
    return NLLS_OK;
}

int enqueue_hess_apply(nlls_ctx* c, int which, double lambda, int nvec, const double* d_v, double* d_y) {
    const int64_t ndof = c->info.ndof;
    if (ndof == 0 || nvec < 1) return NLLS_OK;
    int rc = apply_prepare(c); if (rc != NLLS_OK) return rc;
    rc = apply_classify(c); if (rc != NLLS_OK) return rc;
    ApplyIndex& X = c->app; int chunk = 1;
    rc = apply_scratch(c, X.rec_vec, nvec, chunk); if (rc != NLLS_OK) return rc;
    PhasePair ph(c); int64_t nchunks = 0;
    for (int k0 = 0; k0 < nvec; k0 += chunk, ++nchunks) { const int nk = std::min(chunk, nvec - k0);
        for (size_t g = 0; g < c->groups.size(); ++g) { rc = launch_blocks<APP_HESS>(c, g, which, nk, d_v + (int64_t)k0 * ndof, ndof, X.rec.p + X.gbase_vec[g], X.rec_vec); if (rc != NLLS_OK) return rc; }
        rc = launch_gather(c, false, 0, 0xFFFFFFFFu, X.rec_vec, nk, lambda, d_v + (int64_t)k0 * ndof, d_y + (int64_t)k0 * ndof); if (rc != NLLS_OK) return rc; }
    ph.close(8.0 * (double)nvec * (double)(X.rec_vec + ndof));
    c->app_short = (int64_t)c->blocksizes.size() - X.nlong; c->app_long = X.nlong; c->app_chunks = nchunks;
    return NLLS_OK;
}
// what the products with the Schur complement (nlls_schur_apply.hip) share with this file: the index and its row classes, the record scratch (nvec cut into chunks of
// `chunk` under nlls_ctx::app_scratch_cap), and the block launch of one group on a table of the caller's
int apply_index(nlls_ctx* c) { const int rc = apply_prepare(c); return rc != NLLS_OK ? rc : apply_classify(c); }
int apply_records(nlls_ctx* c, int nvec, int& chunk) { return apply_scratch(c, c->app.rec_vec, nvec, chunk); }
// the diagonal-block records of every group at vars[which] into ApplyIndex::rec (one "vector" of rec_diag doubles): enqueue_hess_block_diag without its gather
int enqueue_diag_blocks(nlls_ctx* c, int which) {
    ApplyIndex& X = c->app; int chunk = 1;
    int rc = apply_scratch(c, X.rec_diag, 1, chunk); if (rc != NLLS_OK) return rc;
    for (size_t g = 0; g < c->groups.size(); ++g) { rc = launch_blocks<APP_DIAG>(c, g, which, 1, nullptr, 0, X.rec.p + X.gbase_diag[g], X.rec_diag); if (rc != NLLS_OK) return rc; }
    return NLLS_OK;
}
// the off-diagonal records of one group (Schur-Jacobi, nlls_schur_apply.hip): the sizes the host index needs, and the launch
bool apply_offd_dims(int kind, int& nd, int& od, int* dof) {
    if (is_dyn_kind(kind)) return false;
    return dispatch_res(kind, [&](auto k) { using S = AppSize<k()>; nd = S::ND; od = S::OD; for (int s = 0; s < S::ND; ++s) dof[s] = S::dof(s); return true; }, false);
}
int enqueue_offd_blocks(nlls_ctx* c, size_t g, int which, double* d_out) { return launch_blocks<APP_OFFD>(c, g, which, 1, nullptr, 0, d_out, 0); }
int apply_need_records(nlls_ctx* c, int64_t doubles) { int chunk = 1; return apply_scratch(c, doubles, 1, chunk); }
int enqueue_hess_blocks(nlls_ctx* c, size_t g, int which, int nvec, const uint32_t* boff, const double* d_in, int64_t in_stride) {
    return launch_blocks<APP_HESS>(c, g, which, nvec, d_in, in_stride, c->app.rec.p + c->app.gbase_vec[g], c->app.rec_vec, boff);
}
int enqueue_jac_apply(nlls_ctx* c, int which, int group, int nvec, const double* d_v, double* d_u) {
    const int64_t ndof = c->info.ndof;
    if (ndof == 0 || nvec < 1) return NLLS_OK;
    int rc = apply_prepare(c); if (rc != NLLS_OK) return rc;
    const Group& G = c->groups[(size_t)group]; AppDims D; app_dims(G.res_kind, D);
    PhasePair ph(c);
    rc = launch_blocks<APP_JAC>(c, (size_t)group, which, nvec, d_v, ndof, d_u, G.ncost * D.m); if (rc != NLLS_OK) return rc;
    ph.close(8.0 * (double)nvec * (double)(G.ncost * D.m));
    c->app_short = c->app_long = 0; c->app_chunks = 1; c->app_scratch = 0;
    return NLLS_OK;
}
int enqueue_jact_apply(nlls_ctx* c, int which, int group, int nvec, const double* d_u, double* d_y) {
    const int64_t ndof = c->info.ndof;
    if (ndof == 0 || nvec < 1) return NLLS_OK;
    int rc = apply_prepare(c); if (rc != NLLS_OK) return rc;
    rc = apply_classify(c); if (rc != NLLS_OK) return rc;
    ApplyIndex& X = c->app; const Group& G = c->groups[(size_t)group]; AppDims D; app_dims(G.res_kind, D);
    const int64_t per = G.ncost * D.p, ulen = G.ncost * D.m; int chunk = 1;
    rc = apply_scratch(c, per, nvec, chunk); if (rc != NLLS_OK) return rc;
    const uint32_t lo = (uint32_t)X.gbase_vec[(size_t)group], hi = (uint32_t)(X.gbase_vec[(size_t)group] + per);
    PhasePair ph(c); int64_t nchunks = 0;
    for (int k0 = 0; k0 < nvec; k0 += chunk, ++nchunks) { const int nk = std::min(chunk, nvec - k0);
        rc = launch_blocks<APP_JACT>(c, (size_t)group, which, nk, d_u + (int64_t)k0 * ulen, ulen, X.rec.p, per); if (rc != NLLS_OK) return rc;
        rc = launch_gather(c, false, lo, hi, per, nk, 0.0, nullptr, d_y + (int64_t)k0 * ndof); if (rc != NLLS_OK) return rc; }
    ph.close(8.0 * (double)nvec * (double)(per + ndof));
    c->app_short = (int64_t)c->blocksizes.size() - X.nlong; c->app_long = X.nlong; c->app_chunks = nchunks;
    return NLLS_OK;
}
int enqueue_hess_block_diag(nlls_ctx* c, int which, double lambda, double* d_out) {
    if (c->info.ndof == 0) return NLLS_OK;
    int rc = apply_prepare(c); if (rc != NLLS_OK) return rc;
    rc = apply_classify(c); if (rc != NLLS_OK) return rc;
    ApplyIndex& X = c->app; int chunk = 1;
    rc = apply_scratch(c, X.rec_diag, 1, chunk); if (rc != NLLS_OK) return rc;
    PhasePair ph(c);
    for (size_t g = 0; g < c->groups.size(); ++g) { rc = launch_blocks<APP_DIAG>(c, g, which, 1, nullptr, 0, X.rec.p + X.gbase_diag[g], X.rec_diag); if (rc != NLLS_OK) return rc; }
    rc = launch_gather(c, true, 0, 0xFFFFFFFFu, X.rec_diag, 1, lambda, nullptr, d_out); if (rc != NLLS_OK) return rc;
    ph.close(8.0 * (double)(X.rec_diag + X.nelem_diag));
    c->app_short = (int64_t)c->blocksizes.size() - X.nlong; c->app_long = X.nlong; c->app_chunks = 1;
    return NLLS_OK;
}

}  // namespace nlls
