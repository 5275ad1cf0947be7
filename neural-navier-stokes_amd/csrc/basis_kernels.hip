// neural_spectral field predictor on gfx950, the fields (the coefficient trajectory: ode_mlp_kernels.hip):
// basis expansion u(x,y,t) = sum_k w_k(t) f_k(x,y) (src/neural_spectral/spectral_ode.py:71-79), the Frobenius loss (:182) and
// their gradients, fused so the [nt, mb, 3, nx, ny] prediction is never materialised for training.
//     coeff [T][K][C], basis [K][C][P], obs / pred [T][C][P]
// One contraction, three kernels -- generic (any K <= 32), packed FMA (K <= 16), matrix cores (K <= 16, gradients only); which one a
// call runs, and with what launch geometry, is decided in ONE place: basis_plan, below the kernels.
#include "nns_common.h"
#include <algorithm>

using namespace nns;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int kMaxK = 32;

// What a pass over the observations computes; the template parameter MODE of the three loss kernels.  r = pred - obs, masked to the real
// pixels and time rows.
enum BasisMode {
    MODE_LOSS = 0,     // *sumsq += sum r^2                                                      (nns_basis_loss_fwd_f32)
    MODE_GRAD = 1,      // gcoeff, gbasis = the gradients for g = scale * r                       (nns_basis_loss_bwd_f32)
    MODE_UPSTREAM = 2,  // the same for g READ from `obs`: an upstream gradient of the
                        // materialised prediction, no prediction computed                      (nns_basis_expand_bwd_f32)
    MODE_FUSED = 3      // *sumsq += sum r^2 AND the gradients for g = r (unscaled), ONE sweep   (nns_basis_loss_fused_f32)
};
// with  gbasis[k][c][p] = sum_t coeff[t][k][c] g[t][c][p]   (registers over all t, written once; atomics when the time axis is split),
//       gcoeff[t][k][c] = sum_p basis[k][c][p] g[t][c][p]   (cross-lane reduction + atomics: always zeroed first).

// a finished gbasis value: the only writer of its address unless the time axis is split over workgroups.  (The other lines the generic and
// the packed kernel have in common -- the coefficient staging loop, the sumsq wave reduction -- stay written out in both: as functions
// they changed the register allocation and schedule of 20 and 11 kernels.)
__device__ __forceinline__ void put_gbasis(float* dst, float v, int nsplit) {
    if (nsplit > 1) atomicAdd(dst, v); else *dst = v;
}

// pred[t][c][p] = sum_k coeff[t][k][c] * basis[k][c][p]      (materialising form, PDEFunc.forward)
__global__ __launch_bounds__(256) void basis_expand_kernel(const float* __restrict__ coeff, const float* __restrict__ basis,
                                                           float* __restrict__ pred, int T, int K, int C, int P) {
    __shared__ float cw[kMaxK];
    const int t = blockIdx.y, c = blockIdx.z;
    if (threadIdx.x < K) cw[threadIdx.x] = coeff[((size_t)t * K + threadIdx.x) * C + c];
    __syncthreads();
    for (int p = blockIdx.x * 256 + threadIdx.x; p < P; p += gridDim.x * 256) {
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(cw[k], basis[((size_t)k * C + c) * P + p], acc);
        pred[((size_t)t * C + c) * P + p] = acc;
    }
}

// One step of the transposing butterfly (see basis_loss_kernel): values [0, 2M) -> [0, M), a lane keeps the half whose index bit matches
// its lane bit and adds its partner's copy.  halve (here, the generic kernel: __shfl_xor) and halve_part (below, the packed kernel: DPP
// moves and v_permlane16_swap_b32) compute the same thing with different instructions.
constexpr int kPart = 32;           // values per butterfly: TT time rows x KMAX coefficients, reduced within each 32-lane half
template <int M>
__device__ __forceinline__ void halve(float (&part)[kPart], int lane) {
    const bool up = (lane & M) != 0;
#pragma unroll
    for (int e = 0; e < M; ++e) {
        const float send = up ? part[e] : part[e + M];
        const float keep = up ? part[e + M] : part[e];
        part[e] = keep + __shfl_xor(send, M);
    }
}

// Fused loss / gradient pass.  A workgroup owns (channel c, a tile of 256*PPT pixels) and walks all T time
// rows: the K basis values of its pixels stay in registers, obs is streamed ONCE (4 B per element -- the
// compulsory traffic), pred is never written.  MODE: the enumeration above.
// PPT pixels per thread (strided by 256): the cross-lane reduction for gcoeff is paid once per PPT pixels.
template <int MODE, int PPT, int KMAX>
__global__ __launch_bounds__(256) void basis_loss_kernel(const float* __restrict__ coeff, const float* __restrict__ basis,
                                                         const float* __restrict__ obs, double* __restrict__ sumsq,
                                                         float* __restrict__ gcoeff, float* __restrict__ gbasis, float scale,
                                                         int T, int K, int C, int P, int TC, int rows_per_split, int nsplit) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // [TC][KMAX] coefficients of this channel for one chunk of time rows, ZERO-PADDED from K to KMAX: the hot loop runs
    // over all KMAX coefficients with no `k < K` guard (guards inside unrolled loops become a branch forest with
    // conservative waits: 125 scalar instructions and 65 % s_waitcnt per row in the first version)
    float* cw = reinterpret_cast<float*>(smem_raw);
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid % kWave;
    const int pbase = blockIdx.x * 256 * PPT + tid;
    // the time axis is split over blockIdx.z so that a launch has >= ~2048 workgroups even when P*C is small
    // (ensembles: T = nt*mb is the long axis); partial gbasis sums are then combined with float atomics
    const int t_lo = blockIdx.z * rows_per_split, t_hi = min(T, t_lo + rows_per_split);
    float fk[PPT][KMAX], gb[PPT][KMAX];
    bool ok[PPT];
    int pix[PPT];                                                     // clamped pixel index: loads never need a mask
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        ok[i] = pbase + 256 * i < P;
        pix[i] = ok[i] ? pbase + 256 * i : P - 1;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { fk[i][k] = (ok[i] && k < K) ? basis[((size_t)k * C + c) * P + pix[i]] : 0.f; gb[i][k] = 0.f; }
    }
    double local = 0.0;
    // gcoeff[t][k][c] = sum over pixels: per-lane partial sums of TT time rows x KMAX coefficients (32 values) are
    // combined by ONE transposing butterfly within each 32-lane half (lane l ends up with its half's total of value
    // l mod 32) and leave in ONE atomic wave-instruction -- not K reductions and K single-lane atomics per time row
    // (63 M atomic instructions at the ensemble shape of BASELINE config 5).
    constexpr int TT = kPart / KMAX;
    float part[kPart];
#pragma unroll
    for (int e = 0; e < kPart; ++e) part[e] = 0.f;
    auto flush_part = [&](int t_first) {
        // recursive halving: at distance m a lane keeps the half of its values whose index bit matches its lane bit
        halve<16>(part, lane); halve<8>(part, lane); halve<4>(part, lane); halve<2>(part, lane); halve<1>(part, lane);
        const int v = lane & (kPart - 1), tt = v / KMAX, k = v % KMAX;
        if (k < K && t_first + tt < t_hi) atomicAdd(&gcoeff[((size_t)(t_first + tt) * K + k) * C + c], part[0]);
#pragma unroll
        for (int e = 0; e < kPart; ++e) part[e] = 0.f;
    };
    for (int t0 = t_lo; t0 < t_hi; t0 += TC) {
        const int tn = min(TC, t_hi - t0);
        const int tnp = (tn + TT - 1) / TT * TT;                     // padded to whole groups: the padding rows have zero coefficients
        __syncthreads();
        for (int e = tid; e < tnp * KMAX; e += 256) {
            const int tt = e / KMAX, k = e % KMAX;
            cw[e] = (tt < tn && k < K) ? coeff[((size_t)(t0 + tt) * K + k) * C + c] : 0.f;
        }
        __syncthreads();
        // observations are requested one row ahead (clamped row index: the extra load of the last row is harmless)
        float obn[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) obn[i] = obs[((size_t)t0 * C + c) * P + pix[i]];
        for (int tt0 = 0; tt0 < tnp; tt0 += TT) {
#pragma unroll
            for (int tq = 0; tq < TT; ++tq) {
                const int tt = tt0 + tq;
                const bool row_ok = tt < tn;                                           // uniform
                float ob[PPT];
#pragma unroll
                for (int i = 0; i < PPT; ++i) ob[i] = obn[i];
                const int tnext = tt + 1 < tn ? tt + 1 : tn - 1;
#pragma unroll
                for (int i = 0; i < PPT; ++i) obn[i] = obs[((size_t)(t0 + tnext) * C + c) * P + pix[i]];
                float w[KMAX];                                                        // this row's coefficients, read once
#pragma unroll
                for (int k4 = 0; k4 < KMAX; k4 += 4) {
                    const float4 q = *reinterpret_cast<const float4*>(cw + tt * KMAX + k4);
                    w[k4] = q.x; w[k4 + 1] = q.y; w[k4 + 2] = q.z; w[k4 + 3] = q.w;
                }
                float g[PPT];
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    float pred = 0.f;
                    if (MODE != MODE_UPSTREAM) {
#pragma unroll
                        for (int k = 0; k < KMAX; ++k) pred = fmaf(w[k], fk[i][k], pred);
                    }
                    const float r = (ok[i] && row_ok) ? (MODE == MODE_UPSTREAM ? ob[i] : pred - ob[i]) : 0.f;
                    if (MODE == MODE_LOSS || MODE == MODE_FUSED) local += (double)r * (double)r;
                    g[i] = (MODE == MODE_UPSTREAM || MODE == MODE_FUSED) ? r : scale * r;
                }
                if (MODE != MODE_LOSS) {
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) {
                        float sred = 0.f;
#pragma unroll
                        for (int i = 0; i < PPT; ++i) { gb[i][k] = fmaf(w[k], g[i], gb[i][k]); sred = fmaf(fk[i][k], g[i], sred); }
                        part[tq * KMAX + k] = sred;
                    }
                }
            }
            if (MODE != MODE_LOSS) flush_part(t0 + tt0);
        }
    }
    if (MODE == MODE_LOSS || MODE == MODE_FUSED) {
        for (int o = kWave / 2; o > 0; o >>= 1) local += __shfl_down(local, o);
        if (lane == 0) atomicAdd(sumsq, local);
    }
    if (MODE != MODE_LOSS) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            if (ok[i]) {
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) put_gbasis(&gbasis[((size_t)k * C + c) * P + pbase + 256 * i], gb[i][k], nsplit);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The same pass for the usual shape (K <= 16, P >= 4096), built around what bounds it on gfx950: arithmetic.  Per
// element the backward needs 3 K FMAs (prediction, gbasis, gcoeff partial); a wave64 v_fma_f32 issues in 4 cycles but
// v_pk_fma_f32 does two lanes' worth in 4.3 (tools/valu_rate_bench.hip), so
//   * every FMA of the hot loop is a v_pk_fma_f32; the packed dimension is the coefficient index (see the kernel);
//   * the coefficients are padded to KMAX in {4, 8, 10, 12, 16} -- the smallest that holds K -- not to 16: at the
//     reference's K = 10 the padding was 37 % of the FMAs;
//   * the per-row gcoeff partials of 32 / KMAX rows (32 values per lane) go through ONE transposing butterfly within each
//     32-lane half (lane l ends with the half's total of value l mod 32) and leave in one atomic wave-instruction.  Its
//     top level -- 16 of the 31 exchange steps -- is v_permlane16_swap_b32 (one VALU instruction swaps the odd / even
//     16-lane rows of two registers in place) instead of two selects and a ds_bpermute per step; the lower levels are
//     DPP moves.  (Inline asm: this ROCm's __builtin_amdgcn_permlane{16,32}_swap returns the same register for both
//     results.)  (A 64-value butterfly over all lanes, v_permlane32_swap on top, was tried: it needs
//     254+ registers and measured slower -- one wave per SIMD or spills.)
// BASELINE config 5 (T = 8192, K = 10, 3 x 256^2): loss backward 4.34 -> 2.92 ms, forward 1.59 -> 1.26 ms.
// ------------------------------------------------------------------------------------------------------------------
typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int kPkPart = 32;          // values per butterfly (one per 32-lane half, 32 / KMAX rows)

// Four independent register pairs per asm block.  A VALU write of an operand within the two preceding issue slots is a
// hazard for these instructions and the compiler does not see inside the block: one leading s_nop 1 covers all four.
#define SWAP4(INSN)                                                                                                  \
    asm volatile("s_nop 1\n\t" INSN " %0, %1\n\t" INSN " %2, %3\n\t" INSN " %4, %5\n\t" INSN " %6, %7"               \
                 : "+v"(a0), "+v"(b0), "+v"(a1), "+v"(b1), "+v"(a2), "+v"(b2), "+v"(a3), "+v"(b3))
__device__ __forceinline__ void swap_rows4(float& a0, float& b0, float& a1, float& b1, float& a2, float& b2, float& a3, float& b3) {
    SWAP4("v_permlane16_swap_b32");                                         // a's odd 16-lane rows <-> b's even rows
}
#undef SWAP4
// values [0, 2M) -> [0, M): the packed kernel's form of halve (see there)
template <int M>
__device__ __forceinline__ void halve_part(float (&part)[kPkPart], int lane) {
    if constexpr (M == 16) {
#pragma unroll
        for (int e = 0; e < M; e += 4) {
            swap_rows4(part[e], part[e + M], part[e + 1], part[e + 1 + M], part[e + 2], part[e + 2 + M], part[e + 3], part[e + 3 + M]);
#pragma unroll
            for (int i = 0; i < 4; ++i) part[e + i] += part[e + i + M];
        }
    } else {
        // lane ^ M within a 16-lane row as DPP moves (VALU, no LDS round trip as ds_bpermute has): quad_perm for M = 1, 2,
        // row_ror:8 for M = 8; M = 4 takes two bank-masked row shifts (lanes with bit 2 clear read lane + 4, the others lane - 4)
        const bool up = (lane & M) != 0;
#pragma unroll
        for (int e = 0; e < M; ++e) {
            const int send = __builtin_bit_cast(int, up ? part[e] : part[e + M]);
            const float keep = up ? part[e + M] : part[e];
            int recv;
            if constexpr (M == 1) recv = __builtin_amdgcn_update_dpp(0, send, 0xB1, 0xF, 0xF, false);          // quad_perm:[1,0,3,2]
            else if constexpr (M == 2) recv = __builtin_amdgcn_update_dpp(0, send, 0x4E, 0xF, 0xF, false);     // quad_perm:[2,3,0,1]
            else if constexpr (M == 8) recv = __builtin_amdgcn_update_dpp(0, send, 0x128, 0xF, 0xF, false);    // row_ror:8
            else {
                recv = __builtin_amdgcn_update_dpp(0, send, 0x104, 0xF, 0x5, false);                            // row_shl:4 -> banks 0, 2
                recv = __builtin_amdgcn_update_dpp(recv, send, 0x114, 0xF, 0xA, false);                         // row_shr:4 -> banks 1, 3
            }
            part[e] = keep + __builtin_bit_cast(float, recv);
        }
    }
}

// time rows per group (kernel and basis_plan): the rows whose gcoeff partials fill one butterfly (gradient modes); the loss has no
// butterfly and takes twice as many (<= 8) per group -- the group is also the depth of the observation prefetch
constexpr int pk_rows_per_butterfly(int kmax) { return kPkPart / kmax < 8 ? kPkPart / kmax : 8; }
constexpr int pk_rows_per_group(int kmax) { return 2 * pk_rows_per_butterfly(kmax) < 8 ? 2 * pk_rows_per_butterfly(kmax) : 8; }

template <int MODE, int KMAX>
__global__ __launch_bounds__(256) void basis_loss_pk_kernel(const float* __restrict__ coeff, const float* __restrict__ basis,
                                                            const float* __restrict__ obs, double* __restrict__ sumsq,
                                                            float* __restrict__ gcoeff, float* __restrict__ gbasis, float scale,
                                                            int T, int K, int C, int P, int TC, int rows_per_split, int nsplit) {
    static_assert(KMAX % 2 == 0 && KMAX <= 16, "coefficient PAIRS");
    constexpr int NP = 4, K2 = KMAX / 2;                               // pixels per thread, coefficient pairs
    // rows per (prefetch) group and per butterfly.  (Prefetching two butterflies ahead in the gradient modes -- TT = pk_rows_per_group --
    // measured the same 3.0 ms at 254 registers instead of 190.)
    constexpr int RB = pk_rows_per_butterfly(KMAX), TT = MODE == MODE_LOSS ? pk_rows_per_group(KMAX) : RB;
    constexpr bool WANT_SS = MODE == MODE_LOSS || MODE == MODE_FUSED;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* cw = reinterpret_cast<float*>(smem_raw);                    // [TC][KMAX], zero-padded (no k < K guard in the hot loop)
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid % kWave;
    const int pbase = blockIdx.x * 1024 + tid;                         // pixels pbase + 256 i, i = 0..3
    const int t_lo = blockIdx.z * rows_per_split, t_hi = min(T, t_lo + rows_per_split);
    // The packed dimension is the COEFFICIENT index: fk[i][q] = (basis[2q], basis[2q+1]) at pixel i.  A row's coefficient
    // pairs then come straight out of LDS as float2 -- no splat -- and the gcoeff partial of a pixel quad is a chain
    // of 4 packed FMAs that ends as the pair (k = 2q, 2q + 1) itself, no horizontal add; only the 4 per-pixel residuals
    // are splat.  (Packing pixel pairs instead cost 3 v_mov per 2 FMAs to build the coefficient splats.)
    v2f fk[NP][K2], gb[NP][K2];
    int pix[NP];
    float okm[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const bool ok = pbase + 256 * i < P;
        pix[i] = ok ? pbase + 256 * i : P - 1;                         // clamped: loads need no mask
        okm[i] = ok ? 1.f : 0.f;
#pragma unroll
        for (int q = 0; q < K2; ++q) {
            const float b0 = (ok && 2 * q < K) ? basis[((size_t)(2 * q) * C + c) * P + pix[i]] : 0.f;
            const float b1 = (ok && 2 * q + 1 < K) ? basis[((size_t)(2 * q + 1) * C + c) * P + pix[i]] : 0.f;
            fk[i][q] = (v2f){b0, b1};
            gb[i][q] = (v2f){0.f, 0.f};
        }
    }
    double local = 0.0;
    float part[kPkPart];
#pragma unroll
    for (int e = 0; e < kPkPart; ++e) part[e] = 0.f;
    auto flush_part = [&](int t_first) {
        halve_part<16>(part, lane); halve_part<8>(part, lane);
        halve_part<4>(part, lane); halve_part<2>(part, lane); halve_part<1>(part, lane);
        const int v = lane % kPkPart, tt = v / KMAX, k = v % KMAX;     // lane l holds the total of value l mod kPkPart = tt * KMAX + k
        if (tt < RB && k < K && t_first + tt < t_hi) atomicAdd(&gcoeff[((size_t)(t_first + tt) * K + k) * C + c], part[0]);
#pragma unroll
        for (int e = 0; e < kPkPart; ++e) part[e] = 0.f;
    };
    for (int t0 = t_lo; t0 < t_hi; t0 += TC) {
        const int tn = min(TC, t_hi - t0);
        const int tnp = (tn + TT - 1) / TT * TT;                       // whole groups: the padding rows have zero coefficients
        __syncthreads();
        for (int e = tid; e < tnp * KMAX; e += 256) {
            const int tt = e / KMAX, k = e % KMAX;
            cw[e] = (tt < tn && k < K) ? coeff[((size_t)(t0 + tt) * K + k) * C + c] : 0.f;
        }
        __syncthreads();
        // Observations are requested one whole GROUP of TT rows ahead (clamped row index: re-reading the last row is
        // harmless).  With one row in flight per wave and two waves per SIMD the pass was latency-bound: 8 KB in
        // flight per CU / ~1.5 us = 1.4 TB/s, which is what it measured.
        float obn[TT][NP];
        auto request = [&](int ttg, auto tqc) {                        // row tq of the group starting at ttg
            constexpr int tq = decltype(tqc)::value;
            const int tt = ttg + tq;
            const size_t row = ((size_t)(t0 + (tt < tn ? tt : tn - 1)) * C + c) * P;
#pragma unroll
            for (int i = 0; i < NP; ++i) obn[tq][i] = obs[row + pix[i]];
        };
        // Every pixel block adds into the SAME gcoeff[t][k][c]; each starts at its own row group and wraps around so that
        // concurrent atomics of different blocks go to different addresses.
        const int ngroups = tnp / TT;
        const int g0 = MODE == MODE_LOSS ? 0 : (int)(((long)blockIdx.x * ngroups) / gridDim.x);
        static_for<0, TT>([&](auto tqc) { request(g0 * TT, tqc); });
        for (int gi = 0; gi < ngroups; ++gi) {
            const int gcur = g0 + gi < ngroups ? g0 + gi : g0 + gi - ngroups;
            const int gnext = gcur + 1 < ngroups ? gcur + 1 : 0;
            const int tt0 = gcur * TT;
            const int ttn = gi + 1 < ngroups ? gnext * TT : tt0;      // the last prefetch re-reads this group
            static_for<0, TT>([&](auto tqc) {
                constexpr int tq = decltype(tqc)::value;
                const int tt = tt0 + tq;
                float ob[NP];
#pragma unroll
                for (int i = 0; i < NP; ++i) ob[i] = obn[tq][i];
                request(ttn, tqc);                                     // rolling: row tq of the next group replaces it at once
                v2f w[K2];                                             // this row's coefficient pairs, read once
#pragma unroll
                for (int q = 0; q < K2; ++q) {
                    const float2 v = *reinterpret_cast<const float2*>(cw + tt * KMAX + 2 * q);
                    w[q] = (v2f){v.x, v.y};
                }
                // No validity masks in the gradient modes: an out-of-range pixel has fk = 0, so it adds 0 to the gcoeff
                // partials, and its gbasis column is never stored; a padding row has w = 0 (nothing into gbasis) and its
                // gcoeff values are dropped at the atomic (row >= t_hi).  MODE_LOSS does need them.
                // (loops are written chain-index innermost: the 4 / K2 independent FMA chains interleave in program
                // order, which the scheduler keeps -- back-to-back dependent packed FMAs each cost a hazard s_nop)
                float g[NP];
                if constexpr (MODE != MODE_UPSTREAM) {
                    v2f pred[NP];
#pragma unroll
                    for (int i = 0; i < NP; ++i) pred[i] = w[0] * fk[i][0];
#pragma unroll
                    for (int q = 1; q < K2; ++q)
#pragma unroll
                        for (int i = 0; i < NP; ++i) pred[i] = __builtin_elementwise_fma(w[q], fk[i][q], pred[i]);
#pragma unroll
                    for (int i = 0; i < NP; ++i) g[i] = (pred[i].x + pred[i].y) - ob[i];
                } else {
#pragma unroll
                    for (int i = 0; i < NP; ++i) g[i] = ob[i];
                }
                if constexpr (WANT_SS) {
                    const float rowm = tt < tn ? 1.f : 0.f;
#pragma unroll
                    for (int i = 0; i < NP; ++i) { const float r = g[i] * (okm[i] * rowm); local += (double)r * (double)r; }
                }
                if constexpr (MODE == MODE_GRAD) {
#pragma unroll
                    for (int i = 0; i < NP; ++i) g[i] *= scale;
                }
                if constexpr (MODE != MODE_LOSS) {
                    v2f sred[K2];
#pragma unroll
                    for (int q = 0; q < K2; ++q) sred[q] = fk[0][q] * (v2f){g[0], g[0]};
#pragma unroll
                    for (int i = 1; i < NP; ++i)
#pragma unroll
                        for (int q = 0; q < K2; ++q) sred[q] = __builtin_elementwise_fma(fk[i][q], (v2f){g[i], g[i]}, sred[q]);
#pragma unroll
                    for (int q = 0; q < K2; ++q) { part[(tq % RB) * KMAX + 2 * q] = sred[q].x; part[(tq % RB) * KMAX + 2 * q + 1] = sred[q].y; }
#pragma unroll
                    for (int i = 0; i < NP; ++i)
#pragma unroll
                        for (int q = 0; q < K2; ++q) gb[i][q] = __builtin_elementwise_fma(w[q], (v2f){g[i], g[i]}, gb[i][q]);
                    if constexpr (tq % RB == RB - 1) flush_part(t0 + tt0 + tq - (RB - 1));
                }
            });
        }
    }
    if constexpr (WANT_SS) {
        for (int o = kWave / 2; o > 0; o >>= 1) local += __shfl_down(local, o);
        if (lane == 0) atomicAdd(sumsq, local);
    }
    if constexpr (MODE != MODE_LOSS) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int px = pbase + 256 * i;
            if (px < P) {
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) put_gbasis(&gbasis[((size_t)k * C + c) * P + px], (k & 1) ? gb[i][k / 2].y : gb[i][k / 2].x, nsplit);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The one-sweep loss + gradient pass on the MATRIX cores (round 2).  The packed-FMA kernel above is bound by the vector rate
// (3 K FMAs per element plus a cross-lane butterfly for the coefficient gradients: 2.9 ms for BASELINE config 5's 6.4 GB of
// observations, 2.3 TB/s).  All three contractions are skinny GEMMs, and v_mfma_f32_16x16x4_f32 is an exact float32 FMA chain
// at the packed-vector peak rate that leaves the vector pipe free:
//     pred  [16 t  x 16 pix] = w  [16 t x KMAX]  f [KMAX x 16 pix]              KQ = KMAX / 4 MFMAs
//     gbasis[KMAX  x 16 pix] += w^T[KMAX x 16 t] g [16 t x 16 pix]              4 MFMAs   (accumulated over all t in registers)
//     gcoeff[16 t  x KMAX ]  += g [16 t x 16 pix] f^T[16 pix x KMAX]            4 MFMAs   (accumulated over the wave's pixel tiles)
// A wave owns NPT = 4 pixel tiles (64 pixels) and walks the time rows in blocks of 16.  Layouts (lane l: lj = l % 16, lg = l / 16):
// the prediction comes out as D[t = 4 lg + r][pix = lj]; the observations are loaded in exactly that layout (a tile is a STRIDED
// pixel set, so that a lane's four tiles are one 16-byte access: four 256-byte row pieces per instruction), so g = pred - obs needs no shuffle, and register r of g IS the B operand of the gbasis product's
// k-step r when the A operand is read from LDS as w[t = 4 lg + r][k = lj] (the contraction order over t is free).  Only the
// coefficient gradient wants t on the lanes: g goes through a 16 x 17 LDS tile once per pixel tile (4 + 4 LDS instructions).
// Every wave parks its gcoeff tile of a time block in LDS (plain stores, no barrier); at the end of a chunk of <= 176 rows the four
// waves' tiles are summed and leave in one burst of global atomics (2.5 wave-instructions per 16 rows x 256 pixels).  Registers: ~100 (4 waves per SIMD), the observations of the next time block are in flight while
// the current one is multiplied.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kMfNPT = 4;                                  // pixel tiles (of 16) per wave
constexpr int kMfTCMax = 176;                               // time rows per chunk at most (11 blocks of 16)
// A 16 x 16 float tile (coefficient blocks, the transposing tile), rows padded to 20 floats, is touched two ways: an instruction covers rows {r, 4 + r, 8 + r, 12 + r} x all columns ([4 lg + r][lj]), or all rows x
// columns {4 s .. 4 s + 3} ([lj][4 s + lg]).  ds_read/write_b32 serve a wave as two 32-lane halves on 32 banks.  Padded to 20 floats per row the
// first pattern is conflict-free, but in the second rows lj and lj + 8 are 160 floats = 5 x 32 banks apart: every such read takes two passes
// (26-29 % of the kernel's LDS cycles are bank conflicts: profiles/r03_mfma_pmc_final.csv).  Round 4 built the conflict-free form VERDICT r3 asked
// for -- no padding, element (t, p) at 16 (t ^ ((t >> 2) & 1)) + (p ^ (t & 14)): a half of the first pattern (rows r, 4 + r) lands in two row
// slots of opposite parity = the two 16-bank halves; a half of the second (16 rows x 2 columns) finds, inside each parity class, 8 rows whose XOR
// keys differ in bits 1..3 -- and MEASURED it (profiles/r04_ab_c5_swizzle.txt, same box, three rounds): conflicts 29 % -> 1.6 % of LDS-active
// cycles, LDS-active cycles 2.13e8 -> 1.53e8 per launch, sweep 1.690 -> 1.713 ms.  The LDS was never the limit (24 % busy): the sweep is bound by
// the issue of its 44 dependent float32 MFMAs per 4 KB (matrix pipe 0.60 busy, 58 % of wave-cycles stalled at issue), and the swizzle's index
// arithmetic costs what the shorter reads save.  Not kept.
constexpr int kMfCwLd = 20;                                 // floats per tile row
__device__ __forceinline__ int mf_tile(int t, int p) { return t * kMfCwLd + p; }
constexpr int mf_quads(int K) { return (K + 3) / 4; }                  // KQ: the kernel's coefficient columns in fours (K <= 16)
constexpr int mf_gacc_ld(int kq) { return kq <= 3 ? 12 : 20; }         // row stride of the parked gcoeff tiles (K <= 12: only 12 columns are kept)
// MODE: the gradient modes of the enumeration above (the loss alone has no matrix-core form)
template <int KQ, int MODE>
// (three waves per SIMD: left to itself the register allocation takes two at K = 10, no spills either way)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void basis_loss_mfma_kernel(const float* __restrict__ coeff, const float* __restrict__ basis,
                                                              const float* __restrict__ obs, double* __restrict__ sumsq,
                                                              float* __restrict__ gcoeff, float* __restrict__ gbasis, float scale,
                                                              int T, int K, int C, int P, int TC, int rows_per_split, int nsplit) {
    constexpr int NPT = kMfNPT, LD = kMfCwLd;
    static_assert(NPT == 4, "a lane's tiles are the four lanes of one 16-byte access");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* cw = reinterpret_cast<float*>(smem_raw);                               // [TC][LD]: w[t][k], zero for k >= K and padding rows
    float* gtb = cw + (size_t)TC * LD;                                            // [4 waves][16][LD]: the transposing tile
    float* gacc = gtb + 4 * 16 * LD;                                              // [TC / 16][4 waves][16][LD]: every wave's gcoeff tile of every time block of the chunk
    const int c = blockIdx.y, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, lj = lane % 16, lg = lane / 16;
    const int pix0 = (blockIdx.x * 4 + wave) * (NPT * 16);
    const int t_lo = blockIdx.z * rows_per_split, t_hi = min(T, t_lo + rows_per_split);
    float* gt = gtb + wave * 16 * LD;
    // invariant operands: the basis functions of the wave's pixels in the two layouts the products need
    // Pixel tile i of the wave is the STRIDED set {pix0 + 4 j + i, j = 0..15}: in the D layout (pix index j = lj) a lane's four tiles are
    // then four consecutive pixels, and the observations of a time row, the basis values and the basis gradients move as 16-byte
    // accesses (P is a multiple of 4 here: checked on the host) -- a wave instruction covers 4 rows x 256 contiguous bytes.
    float Bf[NPT][KQ], fT[NPT][4];
    const int pxl = pix0 + 4 * lj;                                                // this lane's first pixel (D layout)
    const bool pok = pxl < P;                                                     // all four or none (P % 4 == 0)
    const int pcl = pok ? pxl : P - 4;
    const float pm = pok ? 1.f : 0.f;
#pragma unroll
    for (int s = 0; s < KQ; ++s) {
        const int k = 4 * s + lg;
        const float4 v = (k < K && pok) ? *reinterpret_cast<const float4*>(&basis[((size_t)k * C + c) * P + pxl]) : make_float4(0.f, 0.f, 0.f, 0.f);
        Bf[0][s] = v.x; Bf[1][s] = v.y; Bf[2][s] = v.z; Bf[3][s] = v.w;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int pq = pix0 + 4 * (4 * s + lg);                                   // pixel index j = 4 s + lg of every tile
        const float4 v = (lj < K && pq < P) ? *reinterpret_cast<const float4*>(&basis[((size_t)lj * C + c) * P + pq]) : make_float4(0.f, 0.f, 0.f, 0.f);
        fT[0][s] = v.x; fT[1][s] = v.y; fT[2][s] = v.z; fT[3][s] = v.w;
    }
    f32x4 gb[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) gb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    double local = 0.0;
    // The time rows [t_lo, t_hi) are walked in chunks of TC rows (the coefficient block and the gcoeff tiles of a chunk live in LDS);
    // every pixel strip starts at its own chunk and wraps around, so that the bursts of gcoeff atomics at the chunk ends go to
    // different rows.  The next chunk's coefficients are requested into registers when a chunk starts and written to LDS between
    // the two barriers at its end; the observation prefetch runs across the chunk boundaries.
    constexpr int LDG = mf_gacc_ld(KQ);
    constexpr int KM = 4 * KQ;                                                    // coefficient columns that can be non-zero
    constexpr int CNR = (kMfTCMax * KM + 255) / 256;
    const int nchunks = (t_hi - t_lo + TC - 1) / TC;
    const int ci0 = (int)(((long)blockIdx.x * nchunks) / gridDim.x);
    auto chunk_t0 = [&](int j) { int ci = ci0 + j; if (ci >= nchunks) ci -= nchunks; return t_lo + ci * TC; };
    float cn[CNR];
    auto load_coeffs = [&](int t0c) {
        const int tnc = min(TC, t_hi - t0c);
#pragma unroll
        for (int q = 0; q < CNR; ++q) {
            const int e = tid + 256 * q, tt = e / KM, k = e % KM;
            cn[q] = (tt < tnc && k < K) ? coeff[((size_t)(t0c + tt) * K + k) * C + c] : 0.f;
        }
    };
    auto store_coeffs = [&]() {
#pragma unroll
        for (int q = 0; q < CNR; ++q) {
            const int e = tid + 256 * q, tt = e / KM, k = e % KM;
            if (tt < TC) cw[(tt >> 4) * (16 * LD) + mf_tile(tt & 15, k)] = cn[q];
        }
    };
    float4 on[4];                                                                 // row r of the NEXT block: this lane's four consecutive pixels = its four tiles
    auto request = [&](int t0x, int b) {                                          // observations of time block b of the chunk at t0x, D layout
        const int tnx = min(TC, t_hi - t0x);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tt = 16 * b + 4 * lg + r;
            const size_t row = ((size_t)(t0x + (tt < tnx ? tt : tnx - 1)) * C + c) * P;
            const float4 o4 = *reinterpret_cast<const float4*>(&obs[row + pcl]);
            on[r] = o4;
        }
    };
    for (int e = tid; e < TC * LD; e += 256) cw[e] = 0.f;                         // columns >= KM stay zero for the whole kernel
    __syncthreads();
    load_coeffs(chunk_t0(0));
    request(chunk_t0(0), 0);
    store_coeffs();
    __syncthreads();
    for (int j = 0; j < nchunks; ++j) {
        const int t0 = chunk_t0(j);
        const int tn = min(TC, t_hi - t0);
        const int nb = (tn + 15) / 16;                                            // time blocks of this chunk
        const bool more = j + 1 < nchunks;
        const int t0n = more ? chunk_t0(j + 1) : t0;
        if (more) load_coeffs(t0n);
        for (int b = 0; b < nb; ++b) {
            const int tb = 16 * b;
            float o[NPT][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { o[0][r] = on[r].x; o[1][r] = on[r].y; o[2][r] = on[r].z; o[3][r] = on[r].w; }
            if (b + 1 < nb) request(t0, b + 1); else request(t0n, more ? 0 : b);    // the next block is in flight while this one is multiplied
            float Aw[KQ], AwT[4], rm[4];
#pragma unroll
            for (int s = 0; s < KQ; ++s) Aw[s] = cw[tb * LD + mf_tile(lj, 4 * s + lg)];
#pragma unroll
            for (int s = 0; s < 4; ++s) { AwT[s] = cw[tb * LD + mf_tile(4 * lg + s, lj)]; rm[s] = tb + 4 * lg + s < tn ? 1.f : 0.f; }
            f32x4 gc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                float g[4];
                if constexpr (MODE != MODE_UPSTREAM) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < KQ; ++s) acc = mfma4(Aw[s], Bf[i][s], acc);   // pred[t = 4 lg + r][pix = lj]
#pragma unroll
                    for (int r = 0; r < 4; ++r) g[r] = acc[r] - o[i][r];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) g[r] = o[i][r];
                }
                if constexpr (MODE == MODE_FUSED) {
                    float rs = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float mg = g[r] * (rm[r] * pm); rs = __builtin_fmaf(mg, mg, rs); }
                    local += (double)rs;
                }
                if constexpr (MODE == MODE_GRAD) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) g[r] *= scale;
                }
                // (MODE_UPSTREAM: the clamped re-read of a padding row is harmless -- its w is 0 for gbasis and its gcoeff row is dropped at the flush)
                // gbasis: padding rows have w = 0, out-of-range pixels are never stored -- no mask on g
#pragma unroll
                for (int s = 0; s < 4; ++s) gb[i] = mfma4(AwT[s], g[s], gb[i]);
                // gcoeff: g with t on the lanes, through the transposing tile (rows = t, columns = pix)
#pragma unroll
                for (int r = 0; r < 4; ++r) gt[mf_tile(4 * lg + r, lj)] = g[r];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                float gA[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) gA[s] = gt[mf_tile(lj, 4 * s + lg)];
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int s = 0; s < 4; ++s) gc = mfma4(gA[s], fT[i][s], gc);      // gcoeff[t = 4 lg + r][k = lj]
            }
            // this wave's tile of this time block is parked in LDS (plain stores, no barrier: the waves run free inside a chunk;
            // ds_add_f32 into one shared tile measured 1.4 ms of the kernel's 3.0)
            float* ga = gacc + (size_t)(b * 4 + wave) * 16 * LDG;
            if (lj < LDG)
#pragma unroll
            for (int r = 0; r < 4; ++r) ga[(4 * lg + r) * LDG + lj] = gc[r];
        }
        // the chunk's coefficient gradients: the four waves' tiles summed, one burst of global atomics; the next chunk's coefficients in
        __syncthreads();
        for (int e = tid; e < nb * 256; e += 256) {
            const int tt = e / 16, k = e % 16, b = tt / 16, tr = tt % 16;
            if (k < K && tt < tn) {
                const float* ga = gacc + (size_t)(b * 4) * 16 * LDG + tr * LDG + k;
                const float v = (ga[0] + ga[16 * LDG]) + (ga[2 * 16 * LDG] + ga[3 * 16 * LDG]);
                atomicAdd(&gcoeff[((size_t)(t0 + tt) * K + k) * C + c], v);
            }
        }
        if (more) store_coeffs();
        __syncthreads();
    }
    if constexpr (MODE == MODE_FUSED) {
        for (int o = kWave / 2; o > 0; o >>= 1) local += __shfl_down(local, o);
        if (lane == 0) atomicAdd(sumsq, local);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = 4 * lg + r;
        if (pok && k < K) {
            float* dst = &gbasis[((size_t)k * C + c) * P + pxl];
            if (nsplit > 1) {
#pragma unroll
                for (int i = 0; i < NPT; ++i) atomicAdd(dst + i, gb[i][r]);
            } else {
                *reinterpret_cast<float4*>(dst) = make_float4(gb[0][r], gb[1][r], gb[2][r], gb[3][r]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// host side: ONE plan (which kernel, what geometry) and ONE checked launch path for the four passes
// ------------------------------------------------------------------------------------------------------------------
enum BasisKernel { KERNEL_GENERIC, KERNEL_PACKED, KERNEL_MFMA };
struct BasisPlan {
    BasisKernel kernel;
    int width;                          // the kernel's template width: KMAX (generic: kMaxK, packed: 4 .. 16) or KQ (matrix cores: 1 .. 4)
    int TC, rows_per_split, nsplit;     // time rows per LDS chunk, per workgroup along blockIdx.z, and the number of those
    dim3 grid;
    size_t lds;
};

// The time axis is split over blockIdx.z until a launch has ~2048 workgroups (`bxy` = those of one split) even when P * C is small
// (ensembles: T = nt * mb is the long axis), but no finer than `granule` rows, each split whole multiples of `round` rows; the partial
// gbasis sums of the splits are then combined with float atomics.
inline void split_time(BasisPlan& p, int T, int bxy, int granule, int round) {
    const int ns = std::min(std::max(std::min((2048 + bxy - 1) / bxy, (T + granule - 1) / granule), 1), 65535);
    p.rows_per_split = ((T + ns - 1) / ns + round - 1) / round * round;
    p.nsplit = (T + p.rows_per_split - 1) / p.rows_per_split;
}

// Pure: the kernel a pass of mode `mode` over [T][K][C] x [K][C][P] runs and how it is launched.  aligned16: basis, obs and gbasis
// are all 16-byte aligned (the matrix-core kernel moves four pixels per access).
inline BasisPlan basis_plan(int mode, int T, int K, int C, int P, bool aligned16) {
    BasisPlan p;
    const bool mfma = mode != MODE_LOSS && K <= 16 && P % 4 == 0 && aligned16;
    const bool pk = !mfma && K <= 16 && P >= 4096;                         // register budget: 2 * 4 * KMAX floats of basis / gbasis
    p.kernel = mfma ? KERNEL_MFMA : pk ? KERNEL_PACKED : KERNEL_GENERIC;
    const int px = pk ? 1024 : 256;                                        // pixels per workgroup
    const int bx = (P + px - 1) / px;
    if (mfma) {
        p.width = mf_quads(K);
        split_time(p, T, bx * C, 64, 16);                                  // until ~8 workgroups per CU exist (3 run at once), whole 16-row blocks each
        // rows per chunk: coefficients (80 B per row) + the four waves' parked gradient tiles (192 B per row at K <= 12, 320 above) + the
        // transposing tiles must leave room for 3 workgroups per CU (the register budget's occupancy)
        p.TC = std::min(p.rows_per_split, p.width <= 3 ? kMfTCMax : 112);
        p.lds = ((size_t)p.TC * kMfCwLd + 4 * 16 * kMfCwLd + (size_t)(p.TC / 16) * 4 * 16 * mf_gacc_ld(p.width)) * sizeof(float);
    } else {
        p.width = !pk ? kMaxK : K <= 4 ? 4 : K <= 8 ? 8 : K <= 10 ? 10 : K <= 12 ? 12 : 16;      // the kernels pad the coefficients to KMAX
        split_time(p, T, bx * C, 32, 1);
        const int tt = pk ? pk_rows_per_group(p.width) : kPart / p.width;  // TC in whole groups (of the loss: a multiple of the gradient modes')
        p.TC = std::min((p.rows_per_split + tt - 1) / tt * tt, 8192 / p.width / tt * tt);      // <= 32 KB of coefficients per chunk
        p.lds = (size_t)p.TC * p.width * sizeof(float);
    }
    p.grid = dim3(bx, C, p.nsplit);
    return p;
}

// Arguments checked, planned, gradients zeroed (gcoeff is accumulated with atomics always, gbasis too when the time rows are split over
// workgroups: ONE launch for both), launched.
template <int MODE>
int basis_pass(const char* who, const float* coeff, const float* basis, const float* obs, double* sumsq, float* gcoeff, float* gbasis,
               float scale, int T, int K, int C, int P, void* stream) {
    constexpr bool want_ss = MODE == MODE_LOSS || MODE == MODE_FUSED, want_grads = MODE != MODE_LOSS;
    if (!coeff || !basis || !obs || (want_ss && !sumsq) || (want_grads && (!gcoeff || !gbasis)) || T < 1 || K < 1 || C < 1 || P < 1)
        return fail(NNS_ERR_INVALID_ARG, "%s: bad args", who);
    if (K > kMaxK) return fail(NNS_ERR_UNSUPPORTED, "%s: K=%d > %d", who, K, kMaxK);
    if (C > 65535) return fail(NNS_ERR_UNSUPPORTED, "%s: C must be <= 65535", who);
    const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    const BasisPlan p = basis_plan(MODE, T, K, C, P, al16(basis) && al16(obs) && al16(gbasis));
    hipStream_t s = as_stream(stream);
    if constexpr (want_grads) {
        void* const bufs[2] = {gcoeff, gbasis};
        const long bytes[2] = {(long)T * K * C * 4, p.nsplit > 1 ? (long)K * C * P * 4 : 0};
        if (int rc = zero_buffers(bufs, bytes, 2, s); rc != NNS_OK) return rc;
    }
#define LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), p.grid, dim3(256), p.lds, s, coeff, basis, obs, sumsq, gcoeff, gbasis, scale, T, K, C, P, p.TC, p.rows_per_split, p.nsplit)
    if (p.kernel == KERNEL_GENERIC) LAUNCH(basis_loss_kernel<MODE, 1, kMaxK>);
    else if (p.kernel == KERNEL_PACKED) switch (p.width) {
        case 4: LAUNCH(basis_loss_pk_kernel<MODE, 4>); break;
        case 8: LAUNCH(basis_loss_pk_kernel<MODE, 8>); break;
        case 10: LAUNCH(basis_loss_pk_kernel<MODE, 10>); break;
        case 12: LAUNCH(basis_loss_pk_kernel<MODE, 12>); break;
        default: LAUNCH(basis_loss_pk_kernel<MODE, 16>);
    }
    else if constexpr (want_grads) switch (p.width) {
        case 1: LAUNCH(basis_loss_mfma_kernel<1, MODE>); break;
        case 2: LAUNCH(basis_loss_mfma_kernel<2, MODE>); break;
        case 3: LAUNCH(basis_loss_mfma_kernel<3, MODE>); break;
        default: LAUNCH(basis_loss_mfma_kernel<4, MODE>);
    }
#undef LAUNCH
    return check_launch(who);
}

}  // namespace

NNS_API int nns_basis_expand_f32(const float* coeff, const float* basis, float* pred, int T, int K, int C, int P, void* stream) {
    if (!coeff || !basis || !pred || T < 1 || K < 1 || C < 1 || P < 1) return fail(NNS_ERR_INVALID_ARG, "basis_expand: bad args");
    if (K > kMaxK) return fail(NNS_ERR_UNSUPPORTED, "basis_expand: K=%d > %d", K, kMaxK);
    if (T > 65535 || C > 65535) return fail(NNS_ERR_UNSUPPORTED, "basis_expand: T, C must be <= 65535");
    int gx = (P + 255) / 256; if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(basis_expand_kernel, dim3(gx, T, C), dim3(256), 0, as_stream(stream), coeff, basis, pred, T, K, C, P);
    return check_launch("basis_expand");
}

// sumsq (a device double) is ACCUMULATED into: the caller zeroes it (loss = sqrt(sumsq), spectral_ode.py:182).
NNS_API int nns_basis_loss_fwd_f32(const float* coeff, const float* basis, const float* obs, double* sumsq, int T, int K, int C, int P, void* stream) {
    return basis_pass<MODE_LOSS>("basis_loss_fwd", coeff, basis, obs, sumsq, nullptr, nullptr, 0.f, T, K, C, P, stream);
}

// g = scale * (pred - obs) (scale = upstream / loss).  gcoeff [T][K][C] is zeroed here and accumulated with atomics; gbasis is overwritten.
NNS_API int nns_basis_loss_bwd_f32(const float* coeff, const float* basis, const float* obs, float scale, float* gcoeff, float* gbasis,
                                   int T, int K, int C, int P, void* stream) {
    return basis_pass<MODE_GRAD>("basis_loss_bwd", coeff, basis, obs, nullptr, gcoeff, gbasis, scale, T, K, C, P, stream);
}

// ONE sweep over the observations for the loss AND its gradient: *sumsq += sum (pred - obs)^2 (the caller zeroes it),
// gcoeff / gbasis = the gradient of sumsq / 2, i.e. UNSCALED by the upstream factor; d ||.||_2 = (upstream / loss) * these
// (the gradient is linear in that scalar, so the caller applies it afterwards -- obs is read once instead of twice).
NNS_API int nns_basis_loss_fused_f32(const float* coeff, const float* basis, const float* obs, double* sumsq, float* gcoeff, float* gbasis,
                                     int T, int K, int C, int P, void* stream) {
    return basis_pass<MODE_FUSED>("basis_loss_fused", coeff, basis, obs, sumsq, gcoeff, gbasis, 1.f, T, K, C, P, stream);
}

// Backward of nns_basis_expand_f32 for an arbitrary upstream gradient grad_pred [T, C, P].
NNS_API int nns_basis_expand_bwd_f32(const float* coeff, const float* basis, const float* grad_pred, float* gcoeff, float* gbasis,
                                     int T, int K, int C, int P, void* stream) {
    return basis_pass<MODE_UPSTREAM>("basis_expand_bwd", coeff, basis, grad_pred, nullptr, gcoeff, gbasis, 1.f, T, K, C, P, stream);
}
