// Device-side text shared by the row and column kernels of the periodic solver (pspec_kernels.hip): the LDS layout, the kernels' common
// arguments and the row pass's Hermitian fill and kept-mode store.  The rest of what those kernels share is text, included at each site:
// pspec_row_line.inc, pspec_col_tile.inc (the geometry), pspec_stage.inc (the staged forward transform), pspec_field.inc (the field emit).
#pragma once
#include "nns_common.h"
#include "fft_lds.h"

using namespace nns;

namespace {                                // the kernels' namespace: PsArgs is part of their names

constexpr int kT = 256;                    // threads per workgroup (4 waves): more workgroups for the B my1 column lines
constexpr int kW = kT / kWave;

template <int N>
struct PsLds {
    static constexpr int TPF = N / 16, FPW = kWave / TPF, LINES = kW * FPW;
    static constexpr int XB_BYTES = (N + N / 16) * 8;                             // exchange image
    static constexpr int STAGE_BYTES = (N + 16) * 8 + 128;                        // one staged complex line + skew
    static constexpr int LINE_BYTES = ((XB_BYTES > STAGE_BYTES ? XB_BYTES : STAGE_BYTES) + 127) / 128 * 128;
    static constexpr int TAB_BYTES = (N / 2 + Pass2<N>::ENTRIES) * 8;
    static constexpr int TOTAL = TAB_BYTES + LINES * LINE_BYTES;
    static constexpr int SKEW_MOD = LINES < 32 ? LINES : 32, SKEW_DW = 32 / SKEW_MOD;
};

struct PsArgs {
    long nlines;          // row kernel: B nx rows; column kernel: B my1 columns
    long fstride;         // complex elements between the fields of G and of Ph (= B nx my1)
    int my1;              // kept y-wavenumbers
    float kx1, ky1;       // 2 pi / Lx, 2 pi / Ly
    float hnudt;          // -nu dt / 2
    float dt;
    float inv_n;          // 1 / (nx ny)
};

using cf = C2<float>;
__device__ __forceinline__ cf scal(float em, cf z) { return {fmaf(em, z.x, z.x), fmaf(em, z.y, z.y)}; }     // (1 + em) z
__device__ __forceinline__ cf axpy(float a, cf x, cf y) { return {fmaf(a, x.x, y.x), fmaf(a, x.y, y.y)}; }   // a x + y
__device__ __forceinline__ cf imul(float a, cf z) { return {-a * z.y, a * z.x}; }                            // i a z

template <int N>
__device__ __forceinline__ cf* ps_tables(unsigned char* smem) {
    cf* tab = reinterpret_cast<cf*>(smem);
    fill_twiddles<float, N>(tab, threadIdx.x, kT);
    fill_twiddles2<float, N>(tab + N / 2, threadIdx.x, kT);
    __syncthreads();
    return tab;
}

// ---------------------------------------------------------------------------------------------------- row pass (axis y)
// The two helpers of ps_row_kernel and ps_row_adj_kernel.  tid, my1 and valid come by reference, as the lambdas that these were captured them:
// taken by value the row kernels compile to another order of loads, and their code is pinned (tools/isa_listing.py).
// Hermitian fill of two half spectra A, B into Z = A + i B (ifft(Z) = irfft(A) + i irfft(B)); j = 0 takes the real parts
template <int N>
__device__ __forceinline__ void ps_row_load2(const float2* ga, const float2* gb, const int& tid, const int& my1, cf (&z)[16]) {
    constexpr int TPF = PsLds<N>::TPF;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int e = tid + TPF * m;
        z[m] = {0.f, 0.f};
        if (m < 8) {
            if (e < my1) {
                const float2 p = ga[e], q = gb[e];
                z[m] = e == 0 ? cf{p.x, q.x} : cf{p.x - q.y, p.y + q.x};
            }
        } else {
            const int r = N - e;
            if (r < my1) {
                const float2 p = ga[r], q = gb[r];
                z[m] = {p.x + q.y, q.x - p.y};
            }
        }
    }
}
// the kept modes j < my1 of a transformed line
template <int N>
__device__ __forceinline__ void ps_row_store(const cf (&z)[16], float2* o, const int& tid, const int& my1, const bool& valid) {
    constexpr int TPF = PsLds<N>::TPF;
    if (valid) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int e = tid + TPF * m;
            if (e < my1) o[e] = make_float2(z[m].x, z[m].y);
        }
    }
}

}  // namespace
