// nlls_update.hip -- nlls_set_cost_data: new payload records scattered into every device copy of a cost group's data (gfx950).
//
//   the reference's cost objects are mutable and optimize! may be called again on the same problem   src/optimize.jl:5-17
//
// The upload leaves a group's per-block payload in up to 1 + MAX_SLOTS + 2 copies, each in the order its reader wants (Group::data in the caller's order, EntryList::data by
// block row, DenseList::data without the all-fixed blocks, Group::mf_data in elimination order) and keeps, per copy, where block k went (Group::pos_*).  An update is one
// host-to-device copy of the new records into staging of its own and ONE launch that writes every copy of every updated block: a bandwidth-bound scatter of short records.
// Kind-agnostic -- the record length is a run-time argument, no residual template is instantiated -- so a library built with a user header gets it unchanged.
// No atomics (every destination record has one writer: the indices are distinct), no LDS, no scratch memory; stream order is the synchronisation: a sweep enqueued earlier
// on the context's stream reads the old records, everything behind the launch the new ones.
//
// Two regimes, by record length:
//   ndata <= UPD_LANE_MAX   one lane per (updated block, copy): the record moved in 16-byte pieces where ndata is even (every record then starts on a 16-byte boundary: the
//                           buffers are 256-byte aligned), in doubles otherwise.  For the cost-order copy of an update without an index lane i writes record i: the lanes'
//                           stores are back to back, a contiguous copy.
//   ndata >  UPD_LANE_MAX   one wavefront per (updated block, copy, chunk of UPD_WAVE_CHUNK doubles), the lanes striding the chunk: full lines whatever the record's length
//                           (NLLS_RES_DYN_LINEARSQ: up to 512 * 513 doubles per record, 514 chunks).
// The boundary is the memory system's line: 128 bytes = 16 doubles.  Up to there a record lies in one or two lines whichever lane writes it, and a lane per record keeps all
// 64 lanes busy (bundle adjustment: 2 doubles); beyond it a lane of its own would walk its record line by line, 64 lanes in 64 different lines per store, while a wavefront
// writes each line once.
#include "nlls_internal.hpp"

namespace nlls {

constexpr int UPD_LANE_MAX = 16;       // doubles: one cache line
constexpr int UPD_WAVE_CHUNK = 512;    // doubles per wavefront: four 16-byte stores per lane
constexpr int UPD_TPB = 256;

struct UpdCopy { double* data; const uint32_t* pos; };      // pos == nullptr: the cost-order arrays (block k at k)
struct UpdArgs { UpdCopy copy[UPD_MAX_COPIES]; const double* src; const uint32_t* index; int64_t n; int ndata; };   // index: the updated blocks, 0-based (nullptr: 0 .. n - 1)

__device__ __forceinline__ void upd_move(double* __restrict__ d, const double* __restrict__ s, int q0, int q1, int first, int stride, bool pairs) {
    if (pairs) { for (int q = q0 + 2 * first; q < q1; q += 2 * stride) *reinterpret_cast<double2*>(d + q) = *reinterpret_cast<const double2*>(s + q); }
    else { for (int q = q0 + first; q < q1; q += stride) d[q] = s[q]; }
}
// where record i of the staging buffer goes in copy `cp`, or nullptr
__device__ __forceinline__ double* upd_dest(const UpdArgs& a, const UpdCopy& cp, int64_t i) {
    const uint32_t k = a.index ? a.index[i] : (uint32_t)i;
    const uint32_t p = cp.pos ? cp.pos[k] : k;
    return p == UPD_ABSENT ? nullptr : cp.data + (int64_t)p * a.ndata;
}
// grid (ceil(n / 256), copies)
__global__ __launch_bounds__(UPD_TPB) void upd_lane_kernel(const UpdArgs a) {
    const int64_t i = (int64_t)blockIdx.x * UPD_TPB + threadIdx.x; if (i >= a.n) return;
    double* d = upd_dest(a, a.copy[blockIdx.y], i); if (!d) return;
    upd_move(d, a.src + i * a.ndata, 0, a.ndata, 0, 1, (a.ndata & 1) == 0);
}
// grid (ceil(n * nch / 4), copies): wavefront u of the launch takes chunk u % nch of record u / nch
__global__ __launch_bounds__(UPD_TPB) void upd_wave_kernel(const UpdArgs a, int nch) {
    const int64_t u = (int64_t)blockIdx.x * (UPD_TPB / 64) + (threadIdx.x >> 6); const int64_t i = u / nch; if (i >= a.n) return;
    double* d = upd_dest(a, a.copy[blockIdx.y], i); if (!d) return;
    const int q0 = (int)(u - i * nch) * UPD_WAVE_CHUNK, q1 = min(a.ndata, q0 + UPD_WAVE_CHUNK);
    upd_move(d, a.src + i * a.ndata, q0, q1, threadIdx.x & 63, 64, (a.ndata & 1) == 0);
}

// n records at c->upd_stage (and, `indexed`, their blocks at c->upd_index) into every copy of group G
int enqueue_update_scatter(nlls_ctx* c, Group& G, int64_t n, bool indexed) {
    if (!G.pos_on_device) {         // the first update of this upload: the maps go to the device (hipMalloc of their own: nothing of the hot arena moves or grows)
        hipError_t e = hipSuccess;
        for (int s = 0; s < MAX_SLOTS && e == hipSuccess; ++s) if (!G.pos_list[s].empty()) e = G.d_pos_list[s].upload(G.pos_list[s]);
        if (e == hipSuccess && !G.pos_dense.empty()) e = G.d_pos_dense.upload(G.pos_dense);
        if (e == hipSuccess && !G.pos_mf.empty()) e = G.d_pos_mf.upload(G.pos_mf);
        if (e != hipSuccess) return hip_fail(c, e, "nlls_set_cost_data: position maps");
        G.pos_on_device = true;
    }
    UpdArgs a{}; int nc = 0;
    a.copy[nc++] = UpdCopy{G.data.p, nullptr};
    for (int s = 0; s < MAX_SLOTS; ++s) if (!G.pos_list[s].empty() && G.lists[s].data.p) a.copy[nc++] = UpdCopy{G.lists[s].data.p, G.d_pos_list[s].p};
    if (!G.pos_dense.empty() && G.dense.data.p) a.copy[nc++] = UpdCopy{G.dense.data.p, G.d_pos_dense.p};
    if (!G.pos_mf.empty() && G.mf_data.p) a.copy[nc++] = UpdCopy{G.mf_data.p, G.d_pos_mf.p};
    a.src = c->upd_stage.p; a.index = indexed ? c->upd_index.p : nullptr; a.n = n; a.ndata = G.ndata;
    const bool timed = c->phase_on && c->phase_ev.size() >= 10;
    if (timed) (void)hipEventRecord(c->phase_ev[8], c->stream);
    if (G.ndata <= UPD_LANE_MAX) {
        hipLaunchKernelGGL(upd_lane_kernel, dim3((unsigned)((n + UPD_TPB - 1) / UPD_TPB), (unsigned)nc), dim3(UPD_TPB), 0, c->stream, a);
    } else {
        const int nch = (G.ndata + UPD_WAVE_CHUNK - 1) / UPD_WAVE_CHUNK; const int64_t nwg = (n * nch + UPD_TPB / 64 - 1) / (UPD_TPB / 64);
        if (nwg > 0x7FFFFFFFll) { c->err = "nlls_set_cost_data: too many records for one launch"; return NLLS_ERR_UNSUPPORTED; }
        hipLaunchKernelGGL(upd_wave_kernel, dim3((unsigned)nwg, (unsigned)nc), dim3(UPD_TPB), 0, c->stream, a, nch);
    }
    if (timed) { (void)hipEventRecord(c->phase_ev[9], c->stream); c->upd_pending = true; }
    c->upd_copies = nc;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLLS_OK : hip_fail(c, e, "nlls_set_cost_data: scatter launch");
}

}  // namespace nlls
