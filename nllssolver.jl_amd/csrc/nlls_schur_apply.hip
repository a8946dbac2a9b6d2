// nlls_schur_apply.hip -- matrix-free products with the Schur complement of the upload's eliminated set (gfx950):
//   y = S(lambda) v,  S(lambda) = B + lambda I - E (C + lambda I)^-1 E'      nlls_schur_apply
//   s = b_r - E (C + lambda I)^-1 b_e                                        nlls_schur_reduce
//   y = [yr ; (C + lambda I)^-1 (b_e - E' yr)]                               nlls_schur_expand
// with H + lambda I = [[B, E], [E', C]] over (r, e): e the blocks nlls_ctx::is_elim marks (an independent set: C is block diagonal), r the other unfixed blocks.
//
//   the reduced system of the direct solvers      src/linearsolver.jl:20-32 (what nlls_solve factors; here it is applied, never formed)
//
// H is evaluated at the variable set of the call by the block launch of nlls_apply.hip (apply_blocks_kernel, one lane per cost block), never read from A.data, and nothing
// of the blocks is kept between the two passes of a product:
//   pass 1   blocks on [v on the r slots; 0 elsewhere] (table boff1), then a gather over the E ROWS ONLY: t_e = E' v, and -- in the same lane, for a row gathered one lane
//            per entry -- the middle step w_e = (C_e + lambda I)^-1 (0 - t_e).  A lane forms the d sums of its row itself, each in the row's list order, so that every lane of
//            the row holds the same t_e and no lane reads what another lane of the launch has stored.  Rows that take wavefronts leave t_e in SchurIndex::t
//            and a launch of the same kernel over their entries applies the inverse.
//   pass 2   blocks again on [v ; w] (table boff2, the permuted layout of SchurIndex::z), then a gather over the R ROWS ONLY, plus lambda v.
// reduce and expand are the same pieces: w = (C + lambda I)^-1 (-b_e - 0) and pass 2 on [0 ; w] plus b_r; pass 1 on yr and (C + lambda I)^-1 (b_e - t_e).
// The set-up of a call gathers, with the same three kernels in their `diag` form, the diagonal blocks of H + lambda I of the e class (under block Jacobi: of the r class
// too) from 4.11's diagonal-block records, and the factor launch of nlls_pcg.hip inverts them in place; a class nobody asked for is not gathered.  Under Schur-Jacobi
// three kernels of their own subtract, from every reduced block, E (C + lambda I)^-1 E' over its eliminated neighbours before that launch: the diagonal blocks of S.
// Every sum has the order of nlls_apply.hip: a row's incidences in ascending (group, block, slot) order, a wavefront row by lane stride 64 and wave_sum's tree, a cut row
// segment by segment.  No atomics.  The k loops are run-time loops over one body: vector k of a call of many carries the bits of a call of its own, and so does a chunk.
// Built like nlls_apply.hip, WITHOUT -fno-honor-nans / -fno-signed-zeros.
#include <algorithm>

#include "nlls_wave.hpp"

namespace nlls {

// One launch's share of a gather over the rows of one class.  Row `row` has the incidences offs[rowptr[row] .. rowptr[row + 1]) (ApplyIndex), read at rec[o + q].
//   Minv null   y[ostart[row] + q] = sum + coef * add[astart[row] + q]                        (add null: the sum alone)
//   Minv set    y[ostart[row] + q] = sum over k of Minv_row[q, k] * (coef * add[astart[row] + k] - t_k), t_k the row's sum for entry k (rec), or tvec[tstart[row] + k]
//               (sums another launch took), or 0
// The lanes behind the nel entries of the launch place the reduced vector psrc (null: zeros) where the pass behind reads it: unknown j of it at pdst[postart[row] + q].
struct SchurGather {
    const uint32_t* rowptr; const uint32_t* offs; const int32_t* bsz; const uint32_t* dstart;
    const ShortElem* el; int64_t nel; const LongItem* items; int64_t nitems; const BigRow* big; int64_t nbig;
    const double* rec; int64_t rec_stride; int nvec;
    const double* tvec; int64_t t_stride; const uint32_t* tstart;
    double coef; const double* add; int64_t add_stride; const uint32_t* astart;
    const double* Minv;
    double* y; int64_t y_stride; const uint32_t* ostart;
    double* part; int part_w;
    int diag; double lambda;      // diag: the rows' DIAGONAL BLOCKS are gathered (offs, rec: the diagonal-block records; d * d entries a row) and lambda goes on their diagonals
    const double* psrc; int64_t psrc_stride, pn; const uint32_t* perow; const uint32_t* pcstart; const uint32_t* postart; double* pdst; int64_t pdst_stride;
};
NLLS_DEV double schur_row_sum(const SchurGather& a, const double* __restrict__ r, uint32_t p0, uint32_t p1, uint32_t q) {
    double s = 0;
    for (uint32_t p = p0; p < p1; ++p) s += r[a.offs[p] + q];
    return s;
}
NLLS_DEV double schur_tail(const SchurGather& a, int k, uint32_t row, uint32_t q, double s) {
    if (a.diag) { if (q % (uint32_t)(a.bsz[row] + 1) == 0) s += a.lambda; return s; }
    return a.add ? s + a.coef * a.add[(int64_t)k * a.add_stride + a.astart[row] + q] : s;
}
// rows gathered one lane per entry, and the placing lanes
__global__ __launch_bounds__(TPB) void schur_rows_kernel(SchurGather a) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= a.nel) {
        const int64_t j = i - a.nel;
        if (j >= a.pn) return;
        const uint32_t row = a.perow[j]; const int64_t at = (int64_t)a.postart[row] + (j - (int64_t)a.pcstart[row]);
        for (int k = 0; k < a.nvec; ++k) a.pdst[(int64_t)k * a.pdst_stride + at] = a.psrc ? a.psrc[(int64_t)k * a.psrc_stride + j] : 0.0;
        return;
    }
    const ShortElem se = a.el[i]; const uint32_t row = se.row, q = se.q, p0 = a.rowptr[row], p1 = a.rowptr[row + 1];
    for (int k = 0; k < a.nvec; ++k) {
        const double* __restrict__ r = a.rec ? a.rec + (int64_t)k * a.rec_stride : nullptr;
        double out;
        if (!a.Minv) out = schur_tail(a, k, row, q, schur_row_sum(a, r, p0, p1, q));
        else {
            const int32_t d = a.bsz[row];
            const double* __restrict__ m = a.Minv + a.dstart[row] + (int64_t)q * d;      // column q of a symmetric block: contiguous
            out = 0;
            for (int32_t kk = 0; kk < d; ++kk) {
                const double t = r ? schur_row_sum(a, r, p0, p1, (uint32_t)kk) : (a.tvec ? a.tvec[(int64_t)k * a.t_stride + a.tstart[row] + kk] : 0.0);
                const double u = (a.add ? a.coef * a.add[(int64_t)k * a.add_stride + a.astart[row] + kk] : 0.0) - t;
                out += m[kk] * u;
            }
        }
        a.y[(int64_t)k * a.y_stride + a.ostart[row] + q] = out;
    }
}
// rows that take wavefronts: one per item, as apply_gather_long_kernel -- a row of at most APP_SEGMENT incidences is written where it belongs, a segment of a longer one
// leaves its sum in `part`
__global__ __launch_bounds__(TPB) void schur_wave_kernel(SchurGather a) {
    const int64_t w = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (w >= a.nitems) return;
    const int lane = (int)(threadIdx.x & 63);
    const LongItem it = a.items[w]; const uint32_t row = it.row, width = (uint32_t)(a.diag ? a.bsz[row] * a.bsz[row] : a.bsz[row]);
    for (int k = 0; k < a.nvec; ++k) {
        const double* __restrict__ r = a.rec + (int64_t)k * a.rec_stride;
        for (uint32_t q = 0; q < width; ++q) {
            double s = 0;
            for (uint32_t p = it.p0 + lane; p < it.p1; p += 64) s += r[a.offs[p] + q];
            s = wave_sum(s);
            if (lane == 0) { if (it.slot == DEST_NONE) a.y[(int64_t)k * a.y_stride + a.ostart[row] + q] = schur_tail(a, k, row, q, s);
                             else a.part[((int64_t)it.slot * a.nvec + k) * a.part_w + q] = s; }
        }
    }
}
// one lane per (cut row, entry): the row's segments in order
__global__ __launch_bounds__(TPB) void schur_cut_kernel(SchurGather a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t b = t / a.part_w; const uint32_t q = (uint32_t)(t - b * a.part_w);
    if (b >= a.nbig) return;
    const BigRow br = a.big[b];
    if (q >= (uint32_t)(a.diag ? a.bsz[br.row] * a.bsz[br.row] : a.bsz[br.row])) return;
    for (int k = 0; k < a.nvec; ++k) { double s = 0;
        for (uint32_t i = 0; i < br.nslots; ++i) s += a.part[((int64_t)(br.slot0 + i) * a.nvec + k) * a.part_w + q];
        a.y[(int64_t)k * a.y_stride + a.ostart[br.row] + q] = schur_tail(a, k, br.row, q, s); }
}

// ---- the diagonal blocks of S(lambda) (Schur-Jacobi, nlls_schur_block_diag) ---------------------------------------------------------
// Entry (a, b) of reduced block `row`, in place: y[ostart[row] + a + b d] -= sum over the row's pairs of sum_k Ebar[a, k] (sum_l W[k, l] Ebar[b, l]), with W the pair's
// eliminated block's inverse (Minv + wstart[e]) and Ebar[a, k] the pair's terms, entry (a, k) of each (the transpose where SjTerm::tr says so), summed in list order
// BEFORE the product.  y holds the block of B + lambda I the gather in front left there.  Block sizes are run-time values and nothing is indexed by them: Ebar is summed
// again where it is needed, d_e (d_e + 1) sums a pair and entry.  Entries (a, b) and (b, a) are both computed as (min, max): what is subtracted is symmetric to the bit.
struct SjArgs {
    const uint32_t* prow; const SjPair* pairs; const SjTerm* terms; const int32_t* bsz; const uint32_t* wstart;
    const ShortElem* el; int64_t nel; const LongItem* items; int64_t nitems; const BigRow* big; int64_t nbig;
    const double* rec; const double* Minv; double* y; const uint32_t* ostart; double* part; int part_w;
    int ntri;      // entries of the upper triangle of the largest wavefront row: the wavefronts launched per item
};
NLLS_DEV double sj_ebar(const SjArgs& g, uint32_t t0, uint32_t t1, uint32_t a, uint32_t k, uint32_t dr, uint32_t de) {
    double s = 0;
    for (uint32_t t = t0; t < t1; ++t) { const SjTerm m = g.terms[t]; s += g.rec[m.off + (m.tr ? k + a * de : a + k * dr)]; }
    return s;
}
NLLS_DEV double sj_pair(const SjArgs& g, uint32_t p, uint32_t a, uint32_t b, uint32_t dr) {
    const SjPair pr = g.pairs[p]; const uint32_t de = (uint32_t)g.bsz[pr.e];
    const double* __restrict__ w = g.Minv + g.wstart[pr.e];
    double s = 0;
    for (uint32_t k = 0; k < de; ++k) { double u = 0;
        for (uint32_t l = 0; l < de; ++l) u += w[k + l * de] * sj_ebar(g, pr.t0, pr.t1, b, l, dr, de);
        s += sj_ebar(g, pr.t0, pr.t1, a, k, dr, de) * u; }
    return s;
}
// rows subtracted one lane per entry: the row's pairs in order
__global__ __launch_bounds__(TPB) void schur_sj_rows_kernel(SjArgs g) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= g.nel) return;
    const ShortElem se = g.el[i]; const uint32_t row = se.row, dr = (uint32_t)g.bsz[row], a = se.q % dr, b = se.q / dr, lo = a < b ? a : b, hi = a < b ? b : a;
    double s = 0;
    for (uint32_t p = g.prow[row]; p < g.prow[row + 1]; ++p) s += sj_pair(g, p, lo, hi, dr);
    const int64_t o = (int64_t)g.ostart[row] + se.q;
    g.y[o] = g.y[o] - s;
}
// rows that take wavefronts: a wavefront per item AND entry of the upper triangle (entry t lies in column b, row a = t - b (b + 1) / 2), lanes striding the item's
// pairs, lane 0 storing both mirror entries -- a whole row in place, a segment of a cut row to `part`.  The entries of a row are independent sums: taken in sequence by
// one wavefront per item they took 2.13 ms on 1 000 wavefronts at ba_1kx100k, spread like this 1.37 ms (notes/r26.md); an entry's sum, and so its bits, is the same either way.
__global__ __launch_bounds__(TPB) void schur_sj_wave_kernel(SjArgs g) {
    const int64_t w = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (w >= g.nitems * g.ntri) return;
    const int lane = (int)(threadIdx.x & 63);
    const LongItem it = g.items[w / g.ntri]; const uint32_t row = it.row, dr = (uint32_t)g.bsz[row], t = (uint32_t)(w % g.ntri);
    uint32_t b = 0; while ((b + 1) * (b + 2) / 2 <= t) ++b;
    const uint32_t a = t - b * (b + 1) / 2;
    if (b >= dr) return;          // (a row smaller than the largest; the whole wavefront leaves)
    {
        double s = 0;
        for (uint32_t p = it.p0 + lane; p < it.p1; p += 64) s += sj_pair(g, p, a, b, dr);
        s = wave_sum(s);
        if (lane == 0) { const uint32_t q1 = a + b * dr, q2 = b + a * dr;
            if (it.slot == DEST_NONE) { const int64_t o = (int64_t)g.ostart[row];
                g.y[o + q1] = g.y[o + q1] - s;
                if (q2 != q1) g.y[o + q2] = g.y[o + q2] - s; }
            else { double* pt = g.part + (int64_t)it.slot * g.part_w; pt[q1] = s; pt[q2] = s; } }
    }
}
// one lane per (cut row, entry): the row's segments in order
__global__ __launch_bounds__(TPB) void schur_sj_cut_kernel(SjArgs g) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t b = t / g.part_w; const uint32_t q = (uint32_t)(t - b * g.part_w);
    if (b >= g.nbig) return;
    const BigRow br = g.big[b];
    if (q >= (uint32_t)(g.bsz[br.row] * g.bsz[br.row])) return;
    double s = 0;
    for (uint32_t i = 0; i < br.nslots; ++i) s += g.part[(int64_t)(br.slot0 + i) * g.part_w + q];
    const int64_t o = (int64_t)g.ostart[br.row] + q;
    g.y[o] = g.y[o] - s;
}

// ================================================================================================
// host side
// ================================================================================================
namespace {
template <class B>
int schur_need(nlls_ctx* c, B& buf, size_t n, const char* what) {
    if (buf.n >= n && buf.p) return NLLS_OK;
    const hipError_t e = buf.alloc(std::max<size_t>(n, 1)); if (e != hipSuccess) { buf.release(); (void)hipGetLastError(); return hip_fail(c, e, what); }
    return NLLS_OK;
}
// the item lists of both classes under the threshold the context holds now (apply_classify's rule: a row of wave_min incidences or more takes wavefronts)
int schur_classify(nlls_ctx* c) {
    SchurIndex& Z = c->sch;
    const int64_t wm = std::max<int64_t>(c->app_wave_min, 1);
    if (Z.wave_min_built == wm) return NLLS_OK;
    for (SchurClass& K : Z.cls) {
        RowClasses R; classify_rows(c, K.blocks.data(), K.blocks.size(), wm, R);          // (apply_classify's rule, on the class's rows)
        std::vector<ShortElem> sh, le, ds;
        for (const uint32_t b : R.short_rows) { const uint32_t d = (uint32_t)c->blocksizes[b];
            for (uint32_t q = 0; q < d; ++q) sh.push_back(ShortElem{b, q});
            for (uint32_t q = 0; q < d * d; ++q) ds.push_back(ShortElem{b, q}); }
        for (const uint32_t b : R.long_rows) for (uint32_t q = 0; q < (uint32_t)c->blocksizes[b]; ++q) le.push_back(ShortElem{b, q});
        HIPCHK(K.shorts.upload(sh)); HIPCHK(K.longel.upload(le)); HIPCHK(K.dshorts.upload(ds)); HIPCHK(K.items.upload(R.items)); HIPCHK(K.big.upload(R.big));
        K.nshort = (int64_t)sh.size(); K.nlongel = (int64_t)le.size(); K.ndshort = (int64_t)ds.size(); K.nitems = (int64_t)R.items.size(); K.nbig = (int64_t)R.big.size();
        K.nlong = (int64_t)R.long_rows.size(); K.nslots = R.nslots; K.part_w = R.part_w_vec; K.part_w_diag = R.part_w_diag;
    }
    Z.wave_min_built = wm;
    return NLLS_OK;
}
int64_t count_elim(const nlls_ctx* c) {
    if (c->is_elim.size() != c->blocksizes.size()) return 0;
    int64_t n = 0; for (uint8_t e : c->is_elim) n += e != 0;
    return n;
}
SchurGather gather_base(nlls_ctx* c, const SchurClass& K, int nvec) {
    const ApplyIndex& X = c->app;
    SchurGather a{};
    a.rowptr = X.rowptr.p; a.offs = X.off_vec.p; a.bsz = c->d_blocksizes.p; a.dstart = X.start_diag.p;
    a.items = K.items.p; a.nitems = K.nitems; a.big = K.big.p; a.nbig = K.nbig;
    a.rec = X.rec.p; a.rec_stride = X.rec_vec; a.nvec = nvec; a.part = c->sch.part.p; a.part_w = K.part_w;
    return a;
}
// the wavefront rows of a class and its cut rows: sums (and the tail the arguments name) to a.y
void launch_wave_rows(nlls_ctx* c, const SchurGather& a, int64_t& launches) {
    if (a.nitems > 0) { hipLaunchKernelGGL(schur_wave_kernel, dim3((unsigned)((a.nitems + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, c->stream, a); ++launches; }
    if (a.nbig > 0) { hipLaunchKernelGGL(schur_cut_kernel, dim3((unsigned)((a.nbig * a.part_w + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, a); ++launches; }
}
void launch_rows(nlls_ctx* c, const SchurGather& a, int64_t& launches) {
    const int64_t n = a.nel + a.pn;
    if (n > 0) { hipLaunchKernelGGL(schur_rows_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, a); ++launches; }
}
}  // namespace

int schur_check(nlls_ctx* c, const char* name) {
    const int rc = apply_check(c, name, -1, false); if (rc != NLLS_OK) return rc;
    if (count_elim(c) == 0) { c->err = std::string(name) + ": the upload eliminated nothing (a dense system, NLLS_FLAG_NO_SCHUR, or no independent set worth it): there is no reduced system"; return NLLS_ERR_UNSUPPORTED; }
    return NLLS_OK;
}

// The r/e index, once per upload: the classes' blocks, where every block starts in the permuted layout, and the block launch's two tables.
int schur_prepare(nlls_ctx* c) {
    int rc = apply_index(c); if (rc != NLLS_OK) return rc;
    SchurIndex& Z = c->sch; const ApplyIndex& X = c->app;
    if (!Z.ready) {
        const size_t nb = c->blocksizes.size(), ng = c->groups.size(); const int64_t ndof = c->info.ndof;
        std::vector<uint32_t> cstart(nb), blk_at((size_t)ndof, 0), erow; std::vector<int32_t> kb[2]; std::vector<uint32_t> kd[2];
        int64_t nred = 0; for (size_t b = 0; b < nb; ++b) if (!c->is_elim[b]) nred += c->blocksizes[b];
        int64_t at[2] = {0, nred}; uint64_t nd2 = 0;
        for (SchurClass& K : Z.cls) K = SchurClass{};
        for (size_t b = 0; b < nb; ++b) { const int e = c->is_elim[b] ? 1 : 0; const int32_t d = c->blocksizes[b];
            cstart[b] = (uint32_t)at[e]; at[e] += d; blk_at[(size_t)c->boffsets[b]] = (uint32_t)b;
            Z.cls[e].blocks.push_back((uint32_t)b); Z.cls[e].nblk++; Z.cls[e].ndof += d; kb[e].push_back(d); kd[e].push_back((uint32_t)nd2); nd2 += (uint64_t)d * d;
            if (!e) for (int32_t q = 0; q < d; ++q) erow.push_back((uint32_t)b); }
        Z.nred = nred; Z.nedof = ndof - nred;
        Z.boff1.clear(); Z.boff2.clear(); Z.boff1.resize(ng); Z.boff2.resize(ng);
        for (size_t g = 0; g < ng; ++g) { const size_t n = X.boff[g].n; if (!n || !X.boff[g].p) continue;
            std::vector<uint32_t> bo(n), b1(n), b2(n);
            HIPCHK(hipMemcpy(bo.data(), X.boff[g].p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));      // (written once, by apply_prepare)
            for (size_t i = 0; i < n; ++i) {
                if (bo[i] == DEST_NONE) { b1[i] = b2[i] = DEST_NONE; continue; }
                const uint32_t b = blk_at[bo[i]];
                b2[i] = cstart[b]; b1[i] = c->is_elim[b] ? DEST_NONE : cstart[b]; }
            HIPCHK(Z.boff1[g].upload(b1)); HIPCHK(Z.boff2[g].upload(b2)); }
        HIPCHK(Z.cstart.upload(cstart)); HIPCHK(Z.erow_r.upload(erow));
        for (int e = 0; e < 2; ++e) { HIPCHK(Z.cls[e].bsz.upload(kb[e])); HIPCHK(Z.cls[e].dstart.upload(kd[e])); }
        Z.wave_min_built = -1; Z.ready = true;
    }
    return schur_classify(c);
}

// The index of Schur-Jacobi, once per upload (behind schur_prepare): for every reduced block its pairs, for every pair its terms; then the row classes under the
// threshold the context holds now.  Only a cost block's slot pairs with ONE reduced and ONE eliminated variable count: a fixed slot contributes nothing, two reduced
// slots would be off-diagonal fill of S, two eliminated ones do not exist (the set is independent).
namespace {
struct SjHostTerm { uint32_t row, e; SjTerm t; };
int schur_sj_classify(nlls_ctx* c) {
    SchurJacobiIndex& J = c->sch.sj;
    const int64_t wm = std::max<int64_t>(c->app_wave_min, 1);
    if (J.wave_min_built == wm) return NLLS_OK;
    std::vector<uint32_t> rows;                                   // the r rows with something to subtract
    for (const uint32_t b : c->sch.cls[0].blocks) if (J.h_prow[b + 1] > J.h_prow[b]) rows.push_back(b);
    RowClasses R; classify_rows(c, rows.data(), rows.size(), wm, R);      // the products' rule decides lane or wavefront; the items here run over PAIRS, and a row is cut by its TERMS
    std::vector<ShortElem> sh; std::vector<LongItem> items; std::vector<BigRow> big; uint32_t nslots = 0; int part_w = 1, ntri = 1;
    for (const uint32_t b : R.short_rows) { const uint32_t d = (uint32_t)c->blocksizes[b]; for (uint32_t q = 0; q < d * d; ++q) sh.push_back(ShortElem{b, q}); }
    for (const uint32_t b : R.long_rows) { const uint32_t p0 = J.h_prow[b], p1 = J.h_prow[b + 1];
        ntri = std::max(ntri, (int)c->blocksizes[b] * ((int)c->blocksizes[b] + 1) / 2);
        if (p1 == p0 || J.h_pairs[p1 - 1].t1 - J.h_pairs[p0].t0 <= APP_SEGMENT) { items.push_back(LongItem{b, p0, p1, DEST_NONE}); continue; }      // (a row's terms are contiguous)
        BigRow br{b, nslots, 0};                                  // more than APP_SEGMENT terms: a cut row, a segment ends behind the pair that brings its terms to APP_SEGMENT
        for (uint32_t p = p0; p < p1;) { uint32_t q = p, nt = 0;
            while (q < p1 && nt < APP_SEGMENT) { nt += J.h_pairs[q].t1 - J.h_pairs[q].t0; ++q; }
            items.push_back(LongItem{b, p, q, nslots++}); ++br.nslots; p = q; }
        big.push_back(br); part_w = std::max(part_w, (int)c->blocksizes[b] * (int)c->blocksizes[b]); }
    HIPCHK(J.shorts.upload(sh)); HIPCHK(J.items.upload(items)); HIPCHK(J.big.upload(big));
    J.nshort = (int64_t)sh.size(); J.nitems = (int64_t)items.size(); J.nbig = (int64_t)big.size(); J.nslots = nslots; J.part_w = part_w; J.ntri = ntri;
    J.wave_min_built = wm;
    return NLLS_OK;
}
int schur_sj_prepare(nlls_ctx* c) {
    SchurIndex& Z = c->sch; SchurJacobiIndex& J = Z.sj; const ApplyIndex& X = c->app;
    if (!J.ready) {
        const size_t nb = c->blocksizes.size(), ng = c->groups.size(); const int64_t ndof = c->info.ndof;
        std::vector<uint32_t> blk_at((size_t)ndof, 0), rstart(nb, DEST_NONE);
        uint64_t nr2 = 0;
        for (size_t b = 0; b < nb; ++b) { blk_at[(size_t)c->boffsets[b]] = (uint32_t)b;
            if (!c->is_elim[b]) { rstart[b] = (uint32_t)nr2; nr2 += (uint64_t)c->blocksizes[b] * (uint64_t)c->blocksizes[b]; } }
        J.gbase.assign(ng, 0); J.has_offd.assign(ng, 0); uint64_t ro = 0;
        std::vector<SjHostTerm> ht;
        for (size_t g = 0; g < ng; ++g) { const Group& G = c->groups[g]; int nd = 0, od = 0, dof[MAX_SLOTS] = {};
            if (!apply_offd_dims(G.res_kind, nd, od, dof)) { c->err = "the diagonal blocks of S: a dynamic-size kind has no per-block Hessian"; return NLLS_ERR_UNSUPPORTED; }
            J.gbase[g] = (int64_t)ro; J.has_offd[g] = G.ncost > 0 && od > 0;
            const size_t n = (size_t)G.ncost * (size_t)nd; if (!n || !od || !X.boff[g].p) continue;
            if (ro + (uint64_t)G.ncost * (uint64_t)od > 0xFFFFFFF0ull) { c->err = "the diagonal blocks of S: the off-diagonal records exceed 32-bit offsets"; return NLLS_ERR_UNSUPPORTED; }
            std::vector<uint32_t> bo(n);
            HIPCHK(hipMemcpy(bo.data(), X.boff[g].p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));      // (written once, by apply_prepare)
            for (int64_t k = 0; k < G.ncost; ++k) { uint32_t po = 0;
                for (int s = 0; s < nd; ++s) for (int t = s + 1; t < nd; ++t) { const uint32_t at = po; po += (uint32_t)(dof[s] * dof[t]);
                    const uint32_t os = bo[(size_t)k * nd + s], ot = bo[(size_t)k * nd + t];
                    if (os == DEST_NONE || ot == DEST_NONE) continue;
                    const uint32_t bs = blk_at[os], bt = blk_at[ot]; const bool es = c->is_elim[bs] != 0, et = c->is_elim[bt] != 0;
                    if (es == et) continue;
                    // slot s reduced: the stored block, rows of slot s, is E_ie; slot t reduced: it is E_ie'
                    ht.push_back(SjHostTerm{es ? bt : bs, es ? bs : bt, SjTerm{(uint32_t)(ro + (uint64_t)k * od + at), es ? 1u : 0u}}); } }
            ro += (uint64_t)G.ncost * (uint64_t)od; }
        if (ht.size() > 0xFFFFFFF0ull) { c->err = "the diagonal blocks of S: the terms exceed 32-bit offsets"; return NLLS_ERR_UNSUPPORTED; }
        // (ht is in ascending (group, block, slot pair) order: a stable sort by (row, e) keeps that order inside a pair)
        std::stable_sort(ht.begin(), ht.end(), [](const SjHostTerm& x, const SjHostTerm& y) { return x.row != y.row ? x.row < y.row : x.e < y.e; });
        std::vector<SjTerm> terms(ht.size()); J.h_pairs.clear(); J.h_prow.assign(nb + 1, 0);
        for (size_t i = 0; i < ht.size(); ++i) { terms[i] = ht[i].t;
            if (i == 0 || ht[i].row != ht[i - 1].row || ht[i].e != ht[i - 1].e) { J.h_pairs.push_back(SjPair{ht[i].e, (uint32_t)i, (uint32_t)i}); ++J.h_prow[ht[i].row + 1]; }
            J.h_pairs.back().t1 = (uint32_t)i + 1; }
        for (size_t b = 0; b < nb; ++b) J.h_prow[b + 1] += J.h_prow[b];
        J.rec_offd = (int64_t)ro; J.nrd2 = (int64_t)nr2;
        HIPCHK(J.prow.upload(J.h_prow)); HIPCHK(J.pairs.upload(J.h_pairs)); HIPCHK(J.terms.upload(terms)); HIPCHK(J.rstart.upload(rstart));
        J.wave_min_built = -1; J.ready = true;
    }
    return schur_sj_classify(c);
}
}  // namespace

// (C_e + lambda I)^-1 for the e blocks, and what r_blocks asks of the r class: the inverses of the blocks of B + lambda I (block Jacobi), or the blocks of S(lambda)
// (Schur-Jacobi) -- inverted too, or left as they are in d_sout.  One call's order: the diagonal-block records; the e gather and factor; the r gather; the off-diagonal
// records, into the same scratch (the stream orders them behind the gathers); the subtraction; the r factor.
int enqueue_schur_setup(nlls_ctx* c, int which, double lambda, int r_blocks, double* d_Minv, double* d_scal, int64_t* launches, double* d_sout) {
    SchurIndex& Z = c->sch; SchurJacobiIndex& J = Z.sj; const ApplyIndex& X = c->app; const bool sj = r_blocks == SCHUR_R_S;
    int rc;
    if (sj) { rc = schur_sj_prepare(c); if (rc != NLLS_OK) return rc;
              rc = apply_need_records(c, std::max(X.rec_diag, J.rec_offd)); if (rc != NLLS_OK) return rc; }      // (both sets of records before the first launch: nothing is freed under one)
    { size_t pn = 0;
      for (int e = 1; e >= (r_blocks ? 0 : 1); --e) pn = std::max(pn, (size_t)Z.cls[e].nslots * (size_t)Z.cls[e].part_w_diag);
      if (sj) pn = std::max(pn, (size_t)J.nslots * (size_t)J.part_w);
      if (pn > 0) { rc = schur_need(c, Z.part, pn, "products with the Schur complement: partial sums of the cut rows' diagonal blocks"); if (rc != NLLS_OK) return rc; } }
    // 4.11's diagonal-block records of every cost block, then nlls_hess_block_diag's gather over the classes that are wanted alone -- the same sums in the same order, so
    // a block holds the bytes nlls_hess_block_diag returns for it; the blocks of a class nobody asked for are not gathered and stay unwritten
    rc = enqueue_diag_blocks(c, which); if (rc != NLLS_OK) return rc;
    int64_t n = 0; for (const Group& G : c->groups) n += G.ncost > 0;
    double* const rout = d_sout ? d_sout : d_Minv; const uint32_t* const rstart = d_sout ? J.rstart.p : X.start_diag.p;
    for (int e = 1; e >= (r_blocks ? 0 : 1); --e) { const SchurClass& K = Z.cls[e]; if (K.nblk == 0) continue;
        SchurGather g = gather_base(c, K, 1);
        g.offs = X.off_diag.p; g.rec_stride = X.rec_diag; g.diag = 1; g.lambda = lambda; g.part = Z.part.p; g.part_w = K.part_w_diag;
        g.el = K.dshorts.p; g.nel = K.ndshort; g.y = e ? d_Minv : rout; g.y_stride = 0; g.ostart = e ? X.start_diag.p : rstart;
        launch_rows(c, g, n); launch_wave_rows(c, g, n);
        HIPCHK(hipGetLastError());
        if (e == 0 && sj) {          // S_ii = B_ii + lambda I - sum over the row's pairs: the e blocks' inverses are in d_Minv by now
            int64_t extra = 0;
            for (size_t gi = 0; gi < c->groups.size(); ++gi) { if (!J.has_offd[gi]) continue;
                rc = enqueue_offd_blocks(c, gi, which, X.rec.p + J.gbase[gi]); if (rc != NLLS_OK) return rc; ++extra; }
            SjArgs a{};
            a.prow = J.prow.p; a.pairs = J.pairs.p; a.terms = J.terms.p; a.bsz = c->d_blocksizes.p; a.wstart = X.start_diag.p;
            a.el = J.shorts.p; a.nel = J.nshort; a.items = J.items.p; a.nitems = J.nitems; a.big = J.big.p; a.nbig = J.nbig;
            a.rec = X.rec.p; a.Minv = d_Minv; a.y = rout; a.ostart = rstart; a.part = Z.part.p; a.part_w = J.part_w;
            if (a.nel > 0) { hipLaunchKernelGGL(schur_sj_rows_kernel, dim3((unsigned)((a.nel + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, a); ++extra; }
            a.ntri = J.ntri;
            if (a.nitems > 0) { hipLaunchKernelGGL(schur_sj_wave_kernel, dim3((unsigned)((a.nitems * a.ntri + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, c->stream, a); ++extra; }
            if (a.nbig > 0) { hipLaunchKernelGGL(schur_sj_cut_kernel, dim3((unsigned)((a.nbig * a.part_w + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, a); ++extra; }
            HIPCHK(hipGetLastError());
            J.launches = extra; n += extra;
        }
        if (e == 0 && d_sout) continue;          // (nlls_schur_block_diag: the blocks leave unfactored)
        rc = enqueue_block_factor(c, Z.cls[e].bsz.p, Z.cls[e].dstart.p, Z.cls[e].nblk, d_Minv, d_scal); if (rc != NLLS_OK) return rc; ++n; }
    if (launches) *launches += n;
    return NLLS_OK;
}

int enqueue_schur_op(nlls_ctx* c, int mode, int which, double lambda, const double* d_Minv, int nvec, const double* d_a, const double* d_yr, double* d_out) {
    const int64_t ndof = c->info.ndof;
    if (ndof == 0 || nvec < 1) return NLLS_OK;
    int rc = schur_prepare(c); if (rc != NLLS_OK) return rc;
    SchurIndex& Z = c->sch; const ApplyIndex& X = c->app; const SchurClass& R = Z.cls[0]; const SchurClass& E = Z.cls[1];
    const int64_t nred = Z.nred; int chunk = 1;
    rc = apply_records(c, nvec, chunk); if (rc != NLLS_OK) return rc;
    if (mode != SCHUR_EXPAND) { rc = schur_need(c, Z.z, (size_t)(chunk * ndof), "products with the Schur complement: the permuted vectors"); if (rc != NLLS_OK) return rc; }
    if (mode != SCHUR_REDUCE && E.nitems > 0) { rc = schur_need(c, Z.t, (size_t)(chunk * ndof), "products with the Schur complement: the sums of the long eliminated rows"); if (rc != NLLS_OK) return rc; }
    { const size_t pe = (size_t)E.nslots * (size_t)E.part_w, pr = (size_t)R.nslots * (size_t)R.part_w;
      if (pe + pr > 0) { rc = schur_need(c, Z.part, std::max(pe, pr) * (size_t)chunk, "products with the Schur complement: partial sums of the cut rows"); if (rc != NLLS_OK) return rc; } }
    int64_t launches = 0, nchunks = 0;
    const bool timed = c->phase_on && c->phase_ev.size() >= 14;      // the call's launches between phase_ev[12] and [13], as a product of nlls_apply.hip (nlls_get_phase_times [12], [13])
    if (timed) (void)hipEventRecord(c->phase_ev[12], c->stream);
    auto blocks = [&](const std::vector<DevBuf<uint32_t>>& tab, int nk, const double* in, int64_t stride) -> int {
        for (size_t g = 0; g < c->groups.size(); ++g) { if (c->groups[g].ncost <= 0) continue;
            const int r2 = enqueue_hess_blocks(c, g, which, nk, tab[g].p, in, stride); if (r2 != NLLS_OK) return r2; ++launches; }
        return NLLS_OK; };
    for (int k0 = 0; k0 < nvec; k0 += chunk, ++nchunks) { const int nk = std::min(chunk, nvec - k0);
        const double* const full_in = mode == SCHUR_APPLY ? nullptr : d_a + (int64_t)k0 * ndof;                                    // b
        const double* const red_in = mode == SCHUR_APPLY ? d_a + (int64_t)k0 * nred : (mode == SCHUR_EXPAND ? d_yr + (int64_t)k0 * nred : nullptr);   // v; yr
        double* const out = d_out + (int64_t)k0 * (mode == SCHUR_EXPAND ? ndof : nred);
        // ---- pass 1 and the middle step: the e rows -----------------------------------------------------------------------------------------------
        if (mode != SCHUR_REDUCE) { rc = blocks(Z.boff1, nk, red_in, nred); if (rc != NLLS_OK) return rc; }
        SchurGather e = gather_base(c, E, nk);
        e.Minv = d_Minv; e.el = E.shorts.p; e.nel = E.nshort;
        if (mode == SCHUR_REDUCE) e.rec = nullptr;
        if (mode != SCHUR_APPLY) { e.coef = mode == SCHUR_REDUCE ? -1.0 : 1.0; e.add = full_in; e.add_stride = ndof; e.astart = X.start_vec.p; }
        if (mode == SCHUR_EXPAND) { e.y = out; e.y_stride = ndof; e.ostart = X.start_vec.p; }
        else { e.y = Z.z.p; e.y_stride = ndof; e.ostart = Z.cstart.p; }
        e.psrc = red_in; e.psrc_stride = nred; e.pn = nred; e.perow = Z.erow_r.p; e.pcstart = Z.cstart.p; e.postart = e.ostart; e.pdst = e.y; e.pdst_stride = ndof;
        launch_rows(c, e, launches);
        if (E.nitems > 0) {         // the e rows that take wavefronts: their sums to t, then the inverse over their entries
            if (mode != SCHUR_REDUCE) { SchurGather w = gather_base(c, E, nk); w.y = Z.t.p; w.y_stride = ndof; w.ostart = Z.cstart.p; launch_wave_rows(c, w, launches); }
            SchurGather m = e; m.el = E.longel.p; m.nel = E.nlongel; m.pn = 0; m.rec = nullptr;
            if (mode != SCHUR_REDUCE) { m.tvec = Z.t.p; m.t_stride = ndof; m.tstart = Z.cstart.p; }
            launch_rows(c, m, launches);
        }
        if (mode == SCHUR_EXPAND) { HIPCHK(hipGetLastError()); continue; }
        // ---- pass 2: the r rows -----------------------------------------------------------------------------------------------------------------------
        rc = blocks(Z.boff2, nk, Z.z.p, ndof); if (rc != NLLS_OK) return rc;
        SchurGather r = gather_base(c, R, nk);
        r.el = R.shorts.p; r.nel = R.nshort; r.y = out; r.y_stride = nred; r.ostart = Z.cstart.p;
        if (mode == SCHUR_APPLY) { r.coef = lambda; r.add = red_in; r.add_stride = nred; r.astart = Z.cstart.p; }
        else { r.coef = 1.0; r.add = full_in; r.add_stride = ndof; r.astart = X.start_vec.p; }
        launch_rows(c, r, launches); launch_wave_rows(c, r, launches);
        HIPCHK(hipGetLastError());
    }
    if (timed) { (void)hipEventRecord(c->phase_ev[13], c->stream); c->app_pending = true;
                 c->app_bytes = 8.0 * (double)nvec * (double)((mode == SCHUR_APPLY ? 2 : 1) * X.rec_vec + ndof + (mode == SCHUR_EXPAND ? ndof : nred)); }      // records of each pass, the permuted vector, the result
    Z.launches = launches;
    c->app_short = (int64_t)c->blocksizes.size() - E.nlong - R.nlong; c->app_long = E.nlong + R.nlong; c->app_chunks = nchunks;
    return NLLS_OK;
}

}  // namespace nlls
