// nlls_launch.hpp -- what every host section that launches kernels needs, once: the HIP error check, run-time value -> template argument, dynamic LDS above the default.
// Included by nlls_internal.hpp behind NLLS_FOR_EACH_RES (dispatch_res walks that list).
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "nlls_ctx.hpp"

namespace nlls {

// ---- errors: "<expr>: <hipGetErrorString>" in nlls_last_error, NLLS_ERR_HIP to the caller ------------------------------------------------------------------
inline int hip_fail(nlls_ctx* c, hipError_t e, const char* what) { c->err = std::string(what) + ": " + hipGetErrorString(e); return NLLS_ERR_HIP; }
#define HIP_TRY(C, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return nlls::hip_fail(C, e_, #expr); } while (0)
#define HIPCHK(expr) HIP_TRY(c, expr)      // (the context is `c` in every file but nlls_capi.cpp, which names it)

// ---- a run-time value as a template argument: f(Const<V>{}) for the V that matches ---------------------------------------------------------------------------
// Each returns what f returns.  A value outside the list: `fallback` when one is given, else nothing happens (f returns void) -- every call site says what it wants there.
template <int V> using Const = std::integral_constant<int, V>;
template <class F, class... R> auto dispatch_dv(int dv, F&& f, R... fallback) {      // unknowns of an eliminated block on the fast path
    switch (dv) { case 3: return f(Const<3>{}); case 2: return f(Const<2>{}); case 1: return f(Const<1>{}); }      // (3 first, as the if-chains had it: f's kernels keep their order in the code object)
    return (fallback, ...);
}
template <class F, class... R> auto dispatch_nt(int nt, F&& f, R... fallback) {      // 16 x 16 tiles per block of the cyclic reduction (BCR_MAXNT)
    switch (nt) { case 1: return f(Const<1>{}); case 2: return f(Const<2>{}); case 3: return f(Const<3>{}); case 4: return f(Const<4>{}); case 5: return f(Const<5>{}); }
    return (fallback, ...);
}
template <class F, class... R> auto dispatch_res(int kind, F&& f, R... fallback) {   // the residual kinds with compile-time sizes, user kinds included
    switch (kind) {
#define X(K) case K: return f(Const<K>{});
        NLLS_FOR_EACH_RES(X)
#undef X
    }
    return (fallback, ...);
}

// ---- dynamic LDS above the 64 KB every kernel may use unasked -------------------------------------------------------------------------------------------------------
// The attribute belongs to a (device, kernel) pair and every context on the device shares it: a process-wide table of the largest size asked for so far, so that
// the attribute only ever grows.  For the CURRENT device.  Called at upload, which has made the context's device current and knows every size (grant_*_lds below and
// in nlls_bcr.hpp): no launch path asks.
constexpr size_t LDS_UNASKED = 64 * 1024;
inline hipError_t grant_dynamic_lds(const void* kernel, size_t bytes) {
    static std::mutex mtx; static std::map<std::pair<int, const void*>, size_t> granted;
    int dev = 0; if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    const std::lock_guard<std::mutex> lock(mtx);
    size_t& have = granted.try_emplace({dev, kernel}, LDS_UNASKED).first->second;
    if (bytes <= have) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}
template <class K> hipError_t grant_dynamic_lds(K* kernel, size_t bytes) { return grant_dynamic_lds(reinterpret_cast<const void*>(kernel), bytes); }

}  // namespace nlls
