// nlls_records.hpp -- per-lane records written out through a wavefront's LDS slab: shared by the per-block linearisation (nlls_linearize.hip) and the matrix-free
// products (nlls_apply.hip).
#pragma once
#include "nlls_wave.hpp"

namespace nlls {

// ================================================================================================
// record stores
// ================================================================================================
// A lane owns one block and so one record of REC doubles per output (affine bundle adjustment: 18 of J, 9 of g, 81 of H).  Written as out[i * REC + q] the 64 lanes of
// every store instruction hit 64 different lines.  Instead each wavefront stages the records of a sub-batch of its lanes in LDS (per-lane stride padded to an odd
// number of doubles: the lanes' writes of one q fall into different banks) and writes the sub-batch's output range -- contiguous, the lanes' blocks being neighbours in
// the output -- with lane-contiguous 8-byte stores, 512 bytes per instruction.  A record of one double is contiguous as it is; one wider than the slab is stored directly.
// Both forms were measured, and a form that stages only long records: notes/r14.md.
constexpr int LIN_WAVE_SLAB = 1024;                            // doubles of LDS per wavefront: TPB / 64 = 4 wavefronts x 8 KB = 32 KB of static LDS per workgroup
constexpr int lin_stride(int rec) { return rec | 1; }
// lanes of a wavefront whose records are staged at a time; 0: stored directly
constexpr int lin_batch(int rec) { return rec <= 1 || lin_stride(rec) > LIN_WAVE_SLAB ? 0 : (LIN_WAVE_SLAB / lin_stride(rec) < 64 ? LIN_WAVE_SLAB / lin_stride(rec) : 64); }

// a wavefront's own LDS traffic, writes of some lanes then reads by others: served in order, the compiler must not move them across this point (as nlls_mf.hpp's)
NLLS_DEV void lin_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

// The records of the wavefront's `cnt` leading lanes (lane l: record `first + l` of `out`); val(q) is entry q of this lane's record, q a compile-time constant.
// Called by all 64 lanes (cnt is wave-uniform).
template <int REC, class F>
NLLS_DEV void store_records(double* __restrict__ out, int64_t first, int cnt, double* slab, F&& val) {
    constexpr int SB = lin_batch(REC), ST = lin_stride(REC);
    const int lane = (int)(threadIdx.x & 63);
    if constexpr (SB == 0) {
        if (lane < cnt) static_for<REC>([&](auto q) { out[(first + lane) * REC + q()] = val(q); });
    } else {
        for (int b0 = 0; b0 < cnt; b0 += SB) {
            if (lane >= b0 && lane < b0 + SB && lane < cnt) { double* s = slab + (lane - b0) * ST; static_for<REC>([&](auto q) { s[q()] = val(q); }); }
            lin_wave_sync();
            const int nb = (cnt - b0 < SB ? cnt - b0 : SB) * REC;
            double* __restrict__ o = out + (first + b0) * REC;
            for (int t = lane; t < nb; t += 64) { const int rec = t / REC; o[t] = slab[rec * ST + (t - rec * REC)]; }
            lin_wave_sync();
        }
    }
}

}  // namespace nlls
