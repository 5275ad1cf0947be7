// Shared host/device helpers for libnns_hip.so (gfx950 / MI355X only): error reporting, the host launch layer every translation unit
// uses between its C entry points and hipLaunchKernelGGL (stream cast, dynamic-LDS opt-in, CU count, grid cap, FFT size dispatch),
// and a few device helpers (XCD remap, boundary lists, static_for).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "../../include/nns.h"

#define NNS_API extern "C" __attribute__((visibility("default")))

namespace nns {

void set_error(const char* fmt, ...);

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    set_error("%s", buf);
    return code;
}

// Every launch function ends with this: surfaces launch-configuration errors without a host sync.
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(NNS_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return NNS_OK;
}

// ---- host launch layer ----
inline hipStream_t as_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// Raise kernel Kern's dynamic-LDS limit to at least `bytes` (above 64 KB a launch needs the opt-in).  The largest size granted is
// remembered per kernel -- Kern itself is the key: kernels that share a function-pointer type do not share a flag -- and the runtime
// is called only for a larger one: once per process for a fixed-size kernel, once per increase for one sized at run time.  Every later
// launch stays free of non-stream API calls.  Safe against concurrent host threads (the rare slow path is serialised).
template <auto Kern>
inline int lds_opt_in(int bytes, const char* what) {
    static std::atomic<int> granted{0};
    static std::mutex slow;
    if (bytes <= granted.load(std::memory_order_acquire)) return NNS_OK;
    std::lock_guard<std::mutex> lock(slow);
    if (bytes <= granted.load(std::memory_order_relaxed)) return NNS_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return fail(NNS_ERR_LAUNCH, "%s: hipFuncSetAttribute(%d B): %s", what, bytes, hipGetErrorString(e));
    granted.store(bytes, std::memory_order_release);
    return NNS_OK;
}

// CU count of the device, queried once (256, the MI355X's, where the query fails).
inline int device_cus() {
    static const int n = [] { int dev = 0, v = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256; return v; }();
    return n;
}

// Workgroups of a grid-stride launch: one per unit of work up to `cap` (the caps are tuned per kernel and stay at the call sites).
inline unsigned capped_grid(long work, long cap) { return (unsigned)(work < cap ? work : cap); }

// The FFT engine's line lengths: powers of two 64 .. 1024, one kernel instantiation each.
inline bool pow2_in_range(int n) { return n >= 64 && n <= 1024 && (n & (n - 1)) == 0; }
template <typename F>
int dispatch_pow2(int n, const char* what, F&& f) {
    switch (n) {
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        case 1024: return f(std::integral_constant<int, 1024>{});
    }
    return fail(NNS_ERR_UNSUPPORTED, "%s: axis length %d is not a power of two in [64, 1024] (the FFT engine's sizes)", what, n);
}

// bufs[i][0 .. bytes[i]) = 0 for every i, ONE launch per 24 buffers (csrc/optim_kernels.hip); entries with bytes <= 0 are skipped
int zero_buffers(void* const* bufs, const long* bytes, int count, hipStream_t s);

inline bool field_args_ok(int batch, int nx, int ny) { return batch >= 1 && nx >= 3 && ny >= 3; }

constexpr int kWave = 64;          // CDNA4 wavefront
constexpr int kNumXCD = 8;         // MI355X: 8 XCDs, blocks dealt round-robin (blockIdx % 8 = XCD group)

// XCD-aware remap (bijective for any grid size): blocks that share an XCD (same id % 8) get a
// CONTIGUOUS range of logical tiles, so neighbouring tiles share that XCD's L2 (halo rows).
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblocks) {
    const unsigned xcd = bid % kNumXCD, q = nblocks / kNumXCD, r = nblocks % kNumXCD;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + bid / kNumXCD;
}

// Device copy of a boundary list, in the field's arithmetic type.
template <typename T>
struct BcListDev {
    int n;
    int kind[NNS_MAX_BC];
    int side[NNS_MAX_BC];
    T value[NNS_MAX_BC];
    T dx[NNS_MAX_BC];
    T dy[NNS_MAX_BC];
};

template <typename T>
inline int make_bc_dev(const nns_bc_list* h, BcListDev<T>& d) {
    if (!h) return fail(NNS_ERR_INVALID_ARG, "bc list is NULL");
    if (h->n < 0 || h->n > NNS_MAX_BC) return fail(NNS_ERR_INVALID_ARG, "bc list length %d not in [0,%d]", h->n, NNS_MAX_BC);
    d.n = h->n;
    for (int i = 0; i < NNS_MAX_BC; ++i) {
        const bool live = i < h->n;
        d.kind[i] = live ? h->kind[i] : 0;
        d.side[i] = live ? h->side[i] : 0;
        d.value[i] = live ? (T)h->value[i] : (T)0;
        d.dx[i] = live ? (T)h->dx[i] : (T)0;
        d.dy[i] = live ? (T)h->dy[i] : (T)0;
        if (live && (h->kind[i] < 0 || h->kind[i] > 1 || h->side[i] < 0 || h->side[i] > 3))
            return fail(NNS_ERR_INVALID_ARG, "bc entry %d: kind %d / side %d invalid", i, h->kind[i], h->side[i]);
    }
    return NNS_OK;
}

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [I0, I1)
template <int I0, int I1, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I0 < I1) { f(std::integral_constant<int, I0>{}); static_for<I0 + 1, I1>(f); }
}

}  // namespace nns
