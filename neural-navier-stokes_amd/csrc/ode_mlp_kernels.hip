// neural_spectral field predictor on gfx950, the coefficient trajectory (the basis expansion and its loss: basis_kernels.hip):
//   * ODEFunc MLP (src/neural_spectral/spectral_ode.py:14-34: Linear(K,128)-ReLU-Linear(128,128)-ELU-Linear(128,K))
//     integrated with the ANODE fixed-step schemes (src/neural_spectral/anode/scheme.py:21-42,
//     time_stepper.py:35-45: dt = 1/Nt, all Nt states returned) -- ONE persistent kernel per call instead of
//     12 tiny GEMM launches per RK4 step: the three weight matrices live in LDS for the whole integration and
//     the linears run on the matrix cores (v_mfma_f32_16x16x4_f32: f32 in / f32 accumulate, bit-for-bit an
//     fmaf chain, so float32 semantics are kept);
//   * its backward, hand-written: like ANODE's "checkpointing adjoint" (anode/adjoint.py:52-70) it RECOMPUTES
//     each step's stages from the stored states and back-propagates through them; weight gradients are
//     accumulated in MFMA accumulators across all steps and stages and written once;
//   * the adjoint recurrence of the time-parallel form of that backward (ode_adjoint_chain_kernel).
//
// A workgroup (4 waves) owns a tile of 16 batch rows (rows beyond mb are zero padding; gradients of padding
// rows are zero by construction).  MFMA operand maps (cdna_hip_programming.md section 3, 16x16x4 f32):
//   A: lane l holds A[row = l&15][k = l>>4],  B: lane l holds B[k = l>>4][col = l&15],
//   C/D: lane l holds D[row = 4*(l>>4) + r][col = l&15], r = 0..3.
#include "nns_common.h"
#include <cstdlib>

using namespace nns;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int H = 128;            // hidden width of ODEFunc (fixed in the reference)
constexpr int KP = 32;            // padded coefficient count (K <= 32: K = 3 * n_coeffs = 30 in the reference driver)
constexpr int HS = 130;           // LDS row stride of [*][128] images: = 2 (mod 32), so the 16 rows x 2 adjacent columns of an A-fragment or transposed-B read hit 32 distinct banks (round 4; 132 = 4 mod 32 made them 2-way)
constexpr int KS = 34;            // LDS row stride of [*][KP] images (= 2 mod 32, as HS)
constexpr int TB = 16;            // batch rows per workgroup
constexpr int NT = 256;           // threads per workgroup (4 waves)

enum { METHOD_EULER = 0, METHOD_RK2 = 1, METHOD_RK4 = 2 };

// ELU(alpha = 1): z for z > 0, expm1(z) otherwise (ODEFunc, spectral_ode.py:14-34).  Round 3: branch-free, ~14 instructions instead of the
// ~40 of expm1f (on the ODE kernels' critical path once per hidden unit and evaluation): exp(z) - 1 by v_exp_f32 where z <= -0.35 (the
// difference is >= 0.3, no cancellation: <= 5e-7 relative), the Taylor polynomial to z^8 above that (truncation 2e-10 at z = -0.35).
// Read out bit for bit by tests/test_gpu_ode_mlp.py on 2048 values of z in [-110, 2]: 1.25e-7 relative at worst (z = -0.3596), asserted <= 1e-6.
__device__ __forceinline__ float elu1(float z) {
    const float t = __builtin_amdgcn_exp2f(z * 1.44269504088896340736f) - 1.0f;
    float p = 2.48015873015873016e-5f;                       // 1/8!
    p = fmaf(p, z, 1.98412698412698413e-4f);                 // 1/7!
    p = fmaf(p, z, 1.38888888888888894e-3f);
    p = fmaf(p, z, 8.33333333333333322e-3f);
    p = fmaf(p, z, 4.16666666666666644e-2f);
    p = fmaf(p, z, 1.66666666666666657e-1f);
    p = fmaf(p, z, 0.5f);
    p = fmaf(p, z, 1.0f);
    p *= z;
    return z > 0.f ? z : (z > -0.35f ? p : t);
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// D_t[16 x 16] += A[16 x KD] * B_t[KD x 16] for NTILE adjacent column tiles t:  A row-major [16][lda] (LDS);  B row-major [KD][ldb] at column
// n0 + 16 t, or (TRANSB) B[k][col] = Bt[n0 + 16 t + col][k] with Bt row-major.  The operands of EIGHT k-steps are requested before their MFMAs,
// one batch ahead, and the tiles share one read of the A operand (round 3: the first version issued two ds_read_b32 and waited for them in
// front of every MFMA -- an LDS round trip per 32-cycle MFMA: 77 us for ONE backward RK4 step of a 16-row tile, of which 11 are matrix-pipe
// time).
template <int KD, int NTILE, bool TRANSB>
__device__ __forceinline__ void mma_batched(const float* A, int lda, const float* B, int ldb, int n0, f32x4 (&acc)[NTILE], int lane) {
    constexpr int UB = 8, NB = KD / (4 * UB);
    static_assert(KD % (4 * UB) == 0, "k depth in batches of eight k-steps");
    const int r = lane & 15, q = lane >> 4;
    float a[2][UB], b[2][NTILE][UB];
    auto request = [&](int buf, int kb) {
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int k = kb + 4 * u + q;
            a[buf][u] = A[r * lda + k];
#pragma unroll
            for (int t = 0; t < NTILE; ++t) b[buf][t][u] = TRANSB ? B[(n0 + 16 * t + r) * ldb + k] : B[k * ldb + n0 + 16 * t + r];
        }
    };
    // FOUR accumulator chains per wave (k-steps dealt round-robin to NSPLIT partial sums per tile): a dependent v_mfma_f32_16x16x4_f32 issues
    // ~64 cycles after the one it waits for, not 32 -- with two chains one MLP evaluation of a 16-row tile took 9700 cycles for 3100 of MFMA
    // (in-kernel cycle stamps)
    constexpr int NSPLIT = 4 / NTILE;
    f32x4 part[NTILE][NSPLIT];
#pragma unroll
    for (int t = 0; t < NTILE; ++t) {
        part[t][0] = acc[t];
#pragma unroll
        for (int sp = 1; sp < NSPLIT; ++sp) part[t][sp] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    request(0, 0);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        if (nb + 1 < NB) request((nb + 1) & 1, 4 * UB * (nb + 1));
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int t = 0; t < NTILE; ++t) part[t][u % NSPLIT] = mfma4(a[nb & 1][u], b[nb & 1][t][u], part[t][u % NSPLIT]);
    }
#pragma unroll
    for (int t = 0; t < NTILE; ++t) {
        if constexpr (NSPLIT == 2) acc[t] = part[t][0] + part[t][1];
        else acc[t] = (part[t][0] + part[t][1]) + (part[t][2] + part[t][3]);
    }
}
// D[16 x 16] += At^T * B over the 16 batch rows: D[i][n] = sum_b At[b][i0 + i] * B[b][n0 + n]
__device__ __forceinline__ f32x4 mma_atb(const float* At, int lda, int i0, const float* B, int ldb, int n0, f32x4 acc, int lane) {
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int k0 = 0; k0 < TB; k0 += 4) acc = mfma4(At[(k0 + q) * lda + i0 + r], B[(k0 + q) * ldb + n0 + r], acc);
    return acc;
}
__device__ __forceinline__ void store_tile(float* D, int ldd, int n0, f32x4 acc, int lane) {
    const int c = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) D[(r0 + r) * ldd + n0 + c] = acc[r];
}

struct MlpLds {                    // weights transposed to [in][out] (+ padding), resident for the whole kernel
    float* Wt0;   // [KP][HS]
    float* Wt1;   // [H][HS]
    float* Wt2;   // [H][KS]
    float* b0;    // [H]
    float* b1;    // [H]
    float* b2;    // [KP]
};
constexpr int kMlpFloats = KP * HS + H * HS + H * KS + 2 * H + KP;

__device__ __forceinline__ float* carve(float*& p, int n) { float* r = p; p += (n + 3) & ~3; return r; }

__device__ void load_mlp(MlpLds& m, float*& lds, const float* W0, const float* b0, const float* W1, const float* b1,
                         const float* W2, const float* b2, int K, int tid) {
    m.Wt0 = carve(lds, KP * HS); m.Wt1 = carve(lds, H * HS); m.Wt2 = carve(lds, H * KS);
    m.b0 = carve(lds, H); m.b1 = carve(lds, H); m.b2 = carve(lds, KP);
    for (int e = tid; e < KP * H; e += NT) { const int k = e / H, n = e % H; m.Wt0[k * HS + n] = k < K ? W0[n * K + k] : 0.f; }   // W0 [H][K]
    for (int e = tid; e < H * H; e += NT) { const int n = e / H, k = e % H; m.Wt1[k * HS + n] = W1[n * H + k]; }                   // W1 [H][H]
    for (int e = tid; e < KP * H; e += NT) { const int n = e / H, k = e % H; m.Wt2[k * KS + n] = n < K ? W2[n * H + k] : 0.f; }    // W2 [K][H]
    for (int e = tid; e < H; e += NT) { m.b0[e] = b0[e]; m.b1[e] = b1[e]; }
    for (int e = tid; e < KP; e += NT) m.b2[e] = e < K ? b2[e] : 0.f;
}

// F = MLP(S):  S [TB][KS] -> h1 [TB][HS] -> h2 [TB][HS] -> F [TB][KS].  Ends with a barrier.
__device__ void mlp_eval(const MlpLds& m, const float* S, float* h1, float* h2, float* F, int wave, int lane) {
    const int c = lane & 15, r0 = 4 * (lane >> 4);
    {                                                                       // layer 1: 8 column tiles, 2 adjacent ones per wave
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        mma_batched<KP, 2, false>(S, KS, m.Wt0, HS, 32 * wave, acc, lane);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n0 = 16 * (wave * 2 + t);
            const float bb = m.b0[n0 + c];
#pragma unroll
            for (int r = 0; r < 4; ++r) h1[(r0 + r) * HS + n0 + c] = fmaxf(acc[t][r] + bb, 0.f);      // ReLU
        }
    }
    __syncthreads();
    {                                                                       // layer 2
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        mma_batched<H, 2, false>(h1, HS, m.Wt1, HS, 32 * wave, acc, lane);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n0 = 16 * (wave * 2 + t);
            const float bb = m.b1[n0 + c];
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float z = acc[t][r] + bb; h2[(r0 + r) * HS + n0 + c] = elu1(z); }   // ELU(alpha = 1)
        }
    }
    __syncthreads();
    if (wave < KP / 16) {                                                   // layer 3: KP/16 column tiles
        const int n0 = 16 * wave;
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
        mma_batched<H, 1, false>(h2, HS, m.Wt2, KS, n0, acc, lane);
        const float bb = m.b2[n0 + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) F[(r0 + r) * KS + n0 + c] = acc[0][r] + bb;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// forward: out[n] = y_{n+1}, n = 0..Nt-1
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void ode_mlp_fwd_kernel(const float* __restrict__ z0, const float* __restrict__ W0, const float* __restrict__ b0,
                                                         const float* __restrict__ W1, const float* __restrict__ b1,
                                                         const float* __restrict__ W2, const float* __restrict__ b2,
                                                         float* __restrict__ out, int mb, int K, int Nt, int method) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    MlpLds m;
    load_mlp(m, lds, W0, b0, W1, b1, W2, b2, K, tid);
    float* h1 = carve(lds, TB * HS); float* h2 = carve(lds, TB * HS);
    float* Y = carve(lds, TB * KS); float* S = carve(lds, TB * KS); float* F = carve(lds, TB * KS); float* ACC = carve(lds, TB * KS);
    const int row0 = blockIdx.x * TB;
    for (int e = tid; e < TB * KS; e += NT) {
        const int b = e / KS, k = e % KS;
        const float v = (row0 + b < mb && k < K) ? z0[(size_t)(row0 + b) * K + k] : 0.f;
        Y[e] = v; S[e] = v;
    }
    __syncthreads();
    const float dt = 1.f / (float)Nt;
    const float c6 = (float)(1.0 / 6.0), c3 = (float)(1.0 / 3.0);
    const int nstage = method == METHOD_RK4 ? 4 : (method == METHOD_RK2 ? 2 : 1);
    for (int n = 0; n < Nt; ++n) {
        for (int s = 0; s < nstage; ++s) {
            mlp_eval(m, S, h1, h2, F, wave, lane);
            for (int e = tid; e < TB * KS; e += NT) {
                const float k = dt * F[e], y = Y[e];
                if (method == METHOD_EULER) { ACC[e] = y + k; }
                else if (method == METHOD_RK2) { if (s == 0) S[e] = y + 0.5f * k; else ACC[e] = y + k; }
                else {
                    if (s == 0) { ACC[e] = y + c6 * k; S[e] = y + 0.5f * k; }
                    else if (s == 1) { ACC[e] = ACC[e] + c3 * k; S[e] = y + 0.5f * k; }
                    else if (s == 2) { ACC[e] = ACC[e] + c3 * k; S[e] = y + k; }
                    else { ACC[e] = ACC[e] + c6 * k; }
                }
            }
            __syncthreads();
        }
        for (int e = tid; e < TB * KS; e += NT) {
            const int b = e / KS, k = e % KS;
            const float y = ACC[e];
            Y[e] = y; S[e] = y;
            if (row0 + b < mb && k < K) out[((size_t)n * mb + row0 + b) * K + k] = y;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// forward, ONE ROW PER WORKGROUP (round 2).  The integration is Nt dependent steps of 4 (RK4) dependent MLP evaluations; the tile
// kernel above spends 14 us per RK4 step on a 16-row MFMA tile however few of its rows are real -- and PDEFunc integrates ONE shared
// trajectory (spectral_ode.py:69).  Here ONE workgroup owns one batch row and keeps ALL THREE weight matrices in registers: every
// layer is a broadcast read of the activation vector from LDS + an FMA chain per thread, 4 small barriers per evaluation, and batch
// rows run on different CUs.  Plain float32 FMAs (the sum order differs from the MFMA tile's; both are float32 dot products).
// ------------------------------------------------------------------------------------------
constexpr int RT = 256;            // threads per row workgroup: one wave per SIMD
// (Round 4, measured and not kept: EIGHT waves -- a quarter row per thread, the quarters of an output in four adjacent lanes meeting in two DPP adds, two waves
// per SIMD: 324 us per 100 RK4 steps against 296 for this kernel, same box: the three barriers per evaluation get dearer, the shorter FMA chains buy less.)
// Round 3: four waves instead of two.  With 128 threads a thread carried a whole row of W1 -- 128 dependent-issue FMAs per evaluation on
// a SIMD that issues one vector instruction every ~5 cycles to a lone wave: ~3000 cycles per evaluation, 530 us per 100 RK4 steps.  Now
// thread (n, half) holds HALF a row (layer 1: 16 of 32 inputs, layer 2: 64 of 128), the two halves sit in lanes l and l + 32 of one wave and
// meet in one cross-lane add; layer 3 splits its 128 inputs over eight 32-thread groups.
__global__ __launch_bounds__(RT) void ode_mlp_fwd_row_kernel(const float* __restrict__ z0, const float* __restrict__ W0, const float* __restrict__ b0,
                                                             const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ W2, const float* __restrict__ b2,
                                                             float* __restrict__ out, int mb, int K, int Nt, int method) {
    __shared__ __attribute__((aligned(16))) float S[KP], h1[H], h2[H];
    const int t = threadIdx.x, row = blockIdx.x;
    const int n = (t & 31) + 32 * (t >> 6), half = (t >> 5) & 1;   // layers 1, 2: output n, input half
    // layer 3 + the scheme's update: output n3 = 8 wave + o3, inputs 16 g3 .. 16 g3 + 15; the eight partial sums of an output sit in eight
    // ADJACENT lanes and meet in three DPP adds, after which all eight hold F and keep the coefficient's RK state redundantly -- no partial-sum
    // array, no fourth barrier (round 3; s_memtime: layer 3 390 + update 430 of an evaluation's 2200 cycles before)
    const int g3 = t & 7, n3 = 8 * (t >> 6) + ((t >> 3) & 7);
    // Round 4: the dot products run on v_pk_fma_f32 -- weights, activations and partial sums as register PAIRS (even element, odd element), so a
    // thread issues half the vector instructions per evaluation (a lone wave per SIMD issues one every ~5 cycles: the FMA count WAS the time)
    using f2 = float __attribute__((ext_vector_type(2)));
    f2 w0[KP / 4], w1[H / 4], w2[8];
#pragma unroll
    for (int j = 0; j < KP / 2; ++j) { const int jj = KP / 2 * half + j; w0[j / 2][j & 1] = jj < K ? W0[(size_t)n * K + jj] : 0.f; }
#pragma unroll
    for (int j = 0; j < H / 2; ++j) w1[j / 2][j & 1] = W1[(size_t)n * H + H / 2 * half + j];
#pragma unroll
    for (int j = 0; j < 16; ++j) w2[j / 2][j & 1] = n3 < K ? W2[(size_t)n3 * H + 16 * g3 + j] : 0.f;
    auto lo = [](const float4& v) { return f2{v.x, v.y}; };
    auto hi = [](const float4& v) { return f2{v.z, v.w}; };
    const float bias0 = half == 0 ? b0[n] : 0.f, bias1 = half == 0 ? b1[n] : 0.f;
    const float bias2 = n3 < K ? b2[n3] : 0.f;
    float y = n3 < K ? z0[(size_t)row * K + n3] : 0.f, acc = 0.f;       // RK state of coefficient n3 (the same in the eight lanes of its group)
    if (g3 == 0) S[n3] = y;
    __syncthreads();
    const float dt = 1.f / (float)Nt;
    const float c6 = (float)(1.0 / 6.0), c3 = (float)(1.0 / 3.0);
    const int nstage = method == METHOD_RK4 ? 4 : (method == METHOD_RK2 ? 2 : 1);
    // the sum of a value over lanes l and l ^ 32, in both: v_permlane32_swap exchanges the upper half of one register with the lower half of
    // the other, so two copies of z become (z_lo, z_lo) and (z_hi, z_hi).  Inline assembly with its own wait states: the builtin
    // (__builtin_amdgcn_permlane32_swap of a value with itself) came out of hipcc 7.2 as `v84 + v84` after the swap.  ~8 cycles instead of
    // the ds_bpermute round trip (~130) behind __shfl_xor.
    auto half_sum = [](float z) {
        float p0 = z, p1 = z;
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(p0), "+v"(p1));
        return p0 + p1;
    };
    // LDS-only barrier: __syncthreads() also waits for the trajectory store of the step before to be acknowledged (vmcnt(0)), ~1 us per RK step
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    for (int it = 0; it < Nt; ++it) {
        for (int s = 0; s < nstage; ++s) {
            {   // layer 1: K -> 128, ReLU
                f2 a0 = {bias0, 0.f}, a1 = {0.f, 0.f};
                const float* x = S + KP / 2 * half;
                float4 xv[KP / 8];                                         // every read in flight before the first FMA (see layer 2)
#pragma unroll
                for (int j = 0; j < KP / 8; ++j) xv[j] = *reinterpret_cast<const float4*>(x + 4 * j);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < KP / 8; j += 2) {
                    a0 = __builtin_elementwise_fma(w0[2 * j], lo(xv[j]), a0); a0 = __builtin_elementwise_fma(w0[2 * j + 1], hi(xv[j]), a0);
                    a1 = __builtin_elementwise_fma(w0[2 * j + 2], lo(xv[j + 1]), a1); a1 = __builtin_elementwise_fma(w0[2 * j + 3], hi(xv[j + 1]), a1);
                }
                a0 += a1;
                const float z = half_sum(a0.x + a0.y);
                if (half == 0) h1[n] = fmaxf(z, 0.f);
            }
            lds_barrier();
            {   // layer 2: 128 -> 128, ELU(alpha = 1); four independent chains
                f2 a[4] = {f2{bias1, 0.f}, f2{0.f, 0.f}, f2{0.f, 0.f}, f2{0.f, 0.f}};
                const float* x = h1 + H / 2 * half;
                // all sixteen broadcast reads first: left to the compiler they came two at a time, each pair waited for (lgkmcnt(1), lgkmcnt(0))
                // -- eight exposed LDS round trips, 1200 of an evaluation's 2500 cycles (s_memtime)
                float4 xv[H / 8];
#pragma unroll
                for (int j = 0; j < H / 8; ++j) xv[j] = *reinterpret_cast<const float4*>(x + 4 * j);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < H / 8; j += 4) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        a[q] = __builtin_elementwise_fma(w1[2 * (j + q)], lo(xv[j + q]), a[q]);
                        a[q] = __builtin_elementwise_fma(w1[2 * (j + q) + 1], hi(xv[j + q]), a[q]);
                    }
                }
                const f2 a2 = (a[0] + a[1]) + (a[2] + a[3]);
                const float z = half_sum(a2.x + a2.y);
                if (half == 0) h2[n] = elu1(z);
            }
            lds_barrier();
            {   // layer 3: 128 -> K, an eighth of the inputs per lane; then F and the scheme's update of coefficient n3 (scheme.py:21-42)
                f2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
                const float* x = h2 + 16 * g3;
                float4 xv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[j] = *reinterpret_cast<const float4*>(x + 4 * j);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    a0 = __builtin_elementwise_fma(w2[2 * j], lo(xv[j]), a0); a0 = __builtin_elementwise_fma(w2[2 * j + 1], hi(xv[j]), a0);
                    a1 = __builtin_elementwise_fma(w2[2 * j + 2], lo(xv[j + 1]), a1); a1 = __builtin_elementwise_fma(w2[2 * j + 3], hi(xv[j + 1]), a1);
                }
                a0 += a1;
                float f = a0.x + a0.y;
                auto dpp_add = [](float v, auto ctrl) { return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xF, 0xF, false)); };
                f = dpp_add(f, std::integral_constant<int, 0xB1>{});            // quad_perm [1,0,3,2]: lanes g3 ^ 1
                f = dpp_add(f, std::integral_constant<int, 0x4E>{});            // quad_perm [2,3,0,1]: lanes g3 ^ 2
                f = dpp_add(f, std::integral_constant<int, 0x141>{});           // row_half_mirror: a lane of the other quad of the eight (all four of it hold the same sum)
                const float F = f + bias2;
                const float k = dt * F;
                if (method == METHOD_EULER) { acc = y + k; }
                else if (method == METHOD_RK2) { if (s == 0) { if (g3 == 0) S[n3] = y + 0.5f * k; } else acc = y + k; }
                else {
                    if (s == 0) { acc = y + c6 * k; if (g3 == 0) S[n3] = y + 0.5f * k; }
                    else if (s == 1) { acc = acc + c3 * k; if (g3 == 0) S[n3] = y + 0.5f * k; }
                    else if (s == 2) { acc = acc + c3 * k; if (g3 == 0) S[n3] = y + k; }
                    else { acc = acc + c6 * k; }
                }
                if (s == nstage - 1) {
                    y = acc;
                    if (g3 == 0) { S[n3] = y; if (n3 < K) out[((size_t)it * mb + row) * K + n3] = y; }
                }
            }
            lds_barrier();
        }
    }
}

// ------------------------------------------------------------------------------------------
// backward.  work: per workgroup 4 stages x (S [TB][KS] + h1 [TB][HS] + h2 [TB][HS]) floats.
// ------------------------------------------------------------------------------------------
constexpr int kStageFloats = TB * KS + 2 * TB * HS;

__global__ __launch_bounds__(NT) void ode_mlp_bwd_kernel(const float* __restrict__ z0, const float* __restrict__ W0, const float* __restrict__ b0,
                                                         const float* __restrict__ W1, const float* __restrict__ b1,
                                                         const float* __restrict__ W2, const float* __restrict__ b2,
                                                         const float* __restrict__ states, const float* __restrict__ gout,
                                                         float* __restrict__ gz0, float* __restrict__ gW0, float* __restrict__ gb0,
                                                         float* __restrict__ gW1, float* __restrict__ gb1, float* __restrict__ gW2,
                                                         float* __restrict__ gb2, float* __restrict__ work,
                                                         int mb, int K, int Nt, int method, float dt_in) {
    const bool want_pg = gW1 != nullptr;                 // uniform: the Jacobian pass of the time-parallel adjoint wants grad_y only (nns_ode_mlp_bwd_steps_f32 with NULL gW* / gb*)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    MlpLds m;
    load_mlp(m, lds, W0, b0, W1, b1, W2, b2, K, tid);
    float* BA = carve(lds, TB * HS); float* BB = carve(lds, TB * HS); float* BC = carve(lds, TB * HS);
    float* Y = carve(lds, TB * KS); float* S = carve(lds, TB * KS); float* F = carve(lds, TB * KS);
    float* GY = carve(lds, TB * KS); float* GF = carve(lds, TB * KS); float* GS = carve(lds, TB * KS);
    float* GK0 = carve(lds, TB * KS); float* GK1 = carve(lds, TB * KS); float* GK2 = carve(lds, TB * KS);
    float* A = carve(lds, TB * KS);
    float* ws = work + (size_t)blockIdx.x * 4 * kStageFloats;
    const int row0 = blockIdx.x * TB;
    const float dt = dt_in > 0.f ? dt_in : 1.f / (float)Nt;          // dt_in: independent single steps of a longer integration (nns_ode_mlp_bwd_steps_f32)
    const float c6 = (float)(1.0 / 6.0), c3 = (float)(1.0 / 3.0);
    const int nstage = method == METHOD_RK4 ? 4 : (method == METHOD_RK2 ? 2 : 1);

    // weight-gradient accumulators (transposed [in][out] tiles), persistent across steps and stages:
    // gWt1: 8x8 tiles -> wave owns (i-tile it, n-tile nt) with (it*8+nt) % 4 == wave: 16 tiles; gWt0: 2x8 -> 4; gWt2: 8x2 -> 4.
    f32x4 aW1[16], aW0[4], aW2[4];
#pragma unroll
    for (int i = 0; i < 16; ++i) aW1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) { aW0[i] = f32x4{0.f, 0.f, 0.f, 0.f}; aW2[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    float ab0 = 0.f, ab1 = 0.f, ab2 = 0.f;               // bias gradients: thread tid < H owns column tid (tid < KP for b2)

    for (int e = tid; e < TB * KS; e += NT) A[e] = 0.f;
    __syncthreads();

    for (int n = Nt - 1; n >= 0; --n) {
        // adjoint of y_{n+1} += grad of output n; y_n = z0 (n == 0) or states[n-1]
        for (int e = tid; e < TB * KS; e += NT) {
            const int b = e / KS, k = e % KS;
            const bool ok = row0 + b < mb && k < K;
            A[e] += ok ? gout[((size_t)n * mb + row0 + b) * K + k] : 0.f;
            const float y = !ok ? 0.f : (n == 0 ? z0[(size_t)(row0 + b) * K + k] : states[((size_t)(n - 1) * mb + row0 + b) * K + k]);
            Y[e] = y; S[e] = y;
        }
        __syncthreads();
        // ---- recompute the stages, saving stage inputs and activations
        for (int s = 0; s < nstage; ++s) {
            mlp_eval(m, S, BA, BB, F, wave, lane);
            float* w = ws + (size_t)s * kStageFloats;
            for (int e = tid; e < TB * KS; e += NT) w[e] = S[e];
            for (int e = tid; e < TB * HS; e += NT) { w[TB * KS + e] = BA[e]; w[TB * KS + TB * HS + e] = BB[e]; }
            if (s + 1 < nstage) {
                for (int e = tid; e < TB * KS; e += NT) {
                    const float k = dt * F[e], y = Y[e];
                    S[e] = (method == METHOD_RK4 && s == 2) ? y + k : y + 0.5f * k;
                }
            }
            __syncthreads();
        }
        // ---- output adjoints of the stage increments k_s
        for (int e = tid; e < TB * KS; e += NT) {
            const float a = A[e];
            GY[e] = a;
            if (method == METHOD_RK4) { GK0[e] = c6 * a; GK1[e] = c3 * a; GK2[e] = c3 * a; GF[e] = dt * (c6 * a); }   // GF = dt * gk4
            else if (method == METHOD_RK2) { GK0[e] = 0.f; GF[e] = dt * a; }                                          // y' = y + k2
            else { GF[e] = dt * a; }
        }
        __syncthreads();
        for (int s = nstage - 1; s >= 0; --s) {
            const float* w = ws + (size_t)s * kStageFloats;
            for (int e = tid; e < TB * KS; e += NT) S[e] = w[e];
            for (int e = tid; e < TB * HS; e += NT) { BA[e] = w[TB * KS + e]; BB[e] = w[TB * KS + TB * HS + e]; }      // h1, h2
            __syncthreads();
            // layer 3 backward: gWt2[k][n] += h2^T GF ; gb2 += colsum GF ; gh2 = GF W2 -> gz2 = gh2 * elu'(z2)
            if (want_pg) {
#pragma unroll
            for (int t = 0; t < 4; ++t) { const int tile = wave + 4 * t, it = tile / 2, nt = tile % 2; aW2[t] = mma_atb(BB, HS, 16 * it, GF, KS, 16 * nt, aW2[t], lane); }
            if (tid < KP) { float sacc = 0.f; for (int b = 0; b < TB; ++b) sacc += GF[b * KS + tid]; ab2 += sacc; }
            }
            {
                f32x4 acc2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
                mma_batched<KP, 2, true>(GF, KS, m.Wt2, KS, 32 * wave, acc2, lane);     // gh2[b][k] = sum_n GF[b][n] Wt2[k][n]
                const int c = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int k0 = 16 * (wave * 2 + t);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float h = BB[(r0 + r) * HS + k0 + c]; BC[(r0 + r) * HS + k0 + c] = acc2[t][r] * (h > 0.f ? 1.f : h + 1.f); }
                }
            }
            __syncthreads();
            // layer 2 backward: gWt1 += h1^T gz2 ; gb1 += colsum gz2 ; gh1 = gz2 W1 -> gz1 = gh1 * relu'(z1)   (into BB)
            if (want_pg) {
#pragma unroll
            for (int t = 0; t < 16; ++t) { const int tile = wave + 4 * t, it = tile / 8, nt = tile % 8; aW1[t] = mma_atb(BA, HS, 16 * it, BC, HS, 16 * nt, aW1[t], lane); }
            if (tid < H) { float sacc = 0.f; for (int b = 0; b < TB; ++b) sacc += BC[b * HS + tid]; ab1 += sacc; }
            }
            {
                f32x4 acc2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
                mma_batched<H, 2, true>(BC, HS, m.Wt1, HS, 32 * wave, acc2, lane);      // gh1[b][k] = sum_n gz2[b][n] Wt1[k][n]
                const int c = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int k0 = 16 * (wave * 2 + t);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float h = BA[(r0 + r) * HS + k0 + c]; BB[(r0 + r) * HS + k0 + c] = h > 0.f ? acc2[t][r] : 0.f; }
                }
            }
            __syncthreads();
            // layer 1 backward: gWt0 += S^T gz1 ; gb0 += colsum gz1 ; GS = gz1 W0
            if (want_pg) {
#pragma unroll
            for (int t = 0; t < 4; ++t) { const int tile = wave + 4 * t, it = tile / 8, nt = tile % 8; aW0[t] = mma_atb(S, KS, 16 * it, BB, HS, 16 * nt, aW0[t], lane); }
            if (tid < H) { float sacc = 0.f; for (int b = 0; b < TB; ++b) sacc += BB[b * HS + tid]; ab0 += sacc; }
            }
            if (wave < KP / 16) {
                f32x4 acc1[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
                mma_batched<H, 1, true>(BB, HS, m.Wt0, HS, 16 * wave, acc1, lane);      // GS[b][k] = sum_n gz1[b][n] Wt0[k][n]
                store_tile(GS, KS, 16 * wave, acc1[0], lane);
            }
            __syncthreads();
            // ---- scheme bookkeeping: gy += GS; pass GS on to the previous stage's increment; next GF
            for (int e = tid; e < TB * KS; e += NT) {
                const float g = GS[e];
                GY[e] += g;
                if (method == METHOD_RK4) {
                    if (s == 3) { GK2[e] += g; GF[e] = dt * GK2[e]; }                 // S4 = y + k3
                    else if (s == 2) { GK1[e] += 0.5f * g; GF[e] = dt * GK1[e]; }     // S3 = y + k2/2
                    else if (s == 1) { GK0[e] += 0.5f * g; GF[e] = dt * GK0[e]; }     // S2 = y + k1/2
                } else if (method == METHOD_RK2) {
                    if (s == 1) { GK0[e] += 0.5f * g; GF[e] = dt * GK0[e]; }
                }
            }
            __syncthreads();
        }
        for (int e = tid; e < TB * KS; e += NT) A[e] = GY[e];
        __syncthreads();
    }
    // ---- results: grad z0, and the weight/bias gradients (atomics: several batch tiles may contribute)
    for (int e = tid; e < TB * KS; e += NT) {
        const int b = e / KS, k = e % KS;
        if (row0 + b < mb && k < K) gz0[(size_t)(row0 + b) * K + k] = A[e];
    }
    if (!want_pg) return;
    const int c = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 16; ++t) {                          // gW1[n][k] = gWt1[k][n]
        const int tile = wave + 4 * t, it = tile / 8, nt = tile % 8;
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(&gW1[(size_t)(16 * nt + c) * H + 16 * it + r0 + r], aW1[t][r]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {                           // gW0[n][k] (k < K) = gWt0[k][n]
        const int tile = wave + 4 * t, it = tile / 8, nt = tile % 8;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int k = 16 * it + r0 + r; if (k < K) atomicAdd(&gW0[(size_t)(16 * nt + c) * K + k], aW0[t][r]); }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {                           // gW2[n][k] (n < K) = gWt2[k][n]
        const int tile = wave + 4 * t, it = tile / 2, nt = tile % 2;
        const int nn = 16 * nt + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) if (nn < K) atomicAdd(&gW2[(size_t)nn * H + 16 * it + r0 + r], aW2[t][r]);
    }
    if (tid < H) { atomicAdd(&gb0[tid], ab0); atomicAdd(&gb1[tid], ab1); }
    if (tid < K) atomicAdd(&gb2[tid], ab2);
}

// ------------------------------------------------------------------------------------------
// the adjoint recurrence of the time-parallel backward (nns/neural_spectral/anode.py)
// ------------------------------------------------------------------------------------------
// lam[Nt-1] = g[Nt-1];  lam[s-1] = g[s-1] + lam[s] J[s]   (row vectors; J[s][b] = d y_{s+1} / d y_s of row b, [K][K])
// Round 3: the first version (one wave, J read from global memory inside every step) paid an HBM / L2 round trip per step: 2.3 us x 99
// steps for BASELINE config 2.  Now wave 0 walks the steps out of LDS (lam broadcast across the lanes by v_readlane, no barrier inside a
// chunk of steps) while waves 1 .. 3 copy the NEXT chunk's Jacobians and g rows into the other half of LDS, eight wide loads in flight per
// thread.  In LDS a step's matrix has a COMPILE-TIME row stride KC (rows and columns >= K stay zero from the start), so the 32 column reads
// of a step are one base register + immediate offsets: with the runtime stride K the per-row offsets were 32 loop-invariant scalars that the
// compiler spilled to VGPR lanes and re-read every step (197 scalar instructions per step, 0.75 us).
constexpr int kChainThreads = 256, kChainLoaders = kChainThreads - 64;
constexpr int kChainLdsFloats = 18 * 1024;                  // per buffer (two buffers: 144 KiB)
template <int KC>
__global__ __launch_bounds__(kChainThreads) void ode_adjoint_chain_kernel(const float* __restrict__ J, const float* __restrict__ g, float* __restrict__ lam,
                                                                          int Nt, int mb, int K, int steps_per_chunk, int vec4, unsigned mK, unsigned mKK) {
    extern __shared__ __attribute__((aligned(16))) float chain_lds[];
    const int b = blockIdx.x, t = threadIdx.x, KK = K * K;
    constexpr int MS = KC * KC + KC;                          // floats of a step in LDS: the padded matrix, then its g row
    const int bufsz = steps_per_chunk * MS;
    for (int e = t; e < 2 * bufsz; e += kChainThreads) chain_lds[e] = 0.f;
    __syncthreads();
    // chunk c covers steps s_hi(c) = Nt - 1 - c * steps_per_chunk down to s_lo(c) >= 1
    auto chunk_lo = [&](int s_hi) { return s_hi - steps_per_chunk + 1 > 1 ? s_hi - steps_per_chunk + 1 : 1; };
    // n / d for n < 65536 as the high word of n * (2^32 / d + 1): exact (checked for every d <= 4096); the loaders' index arithmetic is on the
    // chunk's critical path (a division is ~40 instructions, four per 16-byte load)
    auto mdiv = [](int n, unsigned m) { return m ? (int)__umulhi((unsigned)n, m) : n; };          // m = 0 stands for d = 1
    auto place = [&](float* buf, int q, int r, float v) { const int i = mdiv(r, mK), jj = r - i * K; buf[q * MS + i * KC + jj] = v; };
    auto load_chunk = [&](int s_hi, float* buf) {            // loader threads only
        const int tl = t - 64, s_lo = chunk_lo(s_hi), ns = s_hi - s_lo + 1;
        if (vec4) {
            const int KK4 = KK / 4, total = ns * KK4;
            for (int base = tl; base < total; base += kChainLoaders * 8) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = base + u * kChainLoaders, ec = e < total ? e : total - 1, q = mdiv(ec, mKK), r4 = ec - q * KK4;
                    v[u] = reinterpret_cast<const float4*>(J + ((size_t)(s_lo + q) * mb + b) * KK)[r4];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = base + u * kChainLoaders;
                    if (e < total) {
                        const int q = mdiv(e, mKK), r = 4 * (e - q * KK4);
                        place(buf, q, r, v[u].x); place(buf, q, r + 1, v[u].y); place(buf, q, r + 2, v[u].z); place(buf, q, r + 3, v[u].w);
                    }
                }
            }
        } else {
            const int total = ns * KK;
            for (int base = tl; base < total; base += kChainLoaders * 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = base + u * kChainLoaders, ec = e < total ? e : total - 1, q = mdiv(ec, mKK), r = ec - q * KK;
                    v[u] = J[((size_t)(s_lo + q) * mb + b) * KK + r];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = base + u * kChainLoaders;
                    if (e < total) { const int q = mdiv(e, mKK); place(buf, q, e - q * KK, v[u]); }
                }
            }
        }
        for (int e = tl; e < ns * K; e += kChainLoaders) { const int q = e / K, j = e - q * K; buf[q * MS + KC * KC + j] = g[((size_t)(s_lo + q - 1) * mb + b) * K + j]; }
    };
    float l = 0.f;
    if (t < 64) {
        l = t < K ? g[((size_t)(Nt - 1) * mb + b) * K + t] : 0.f;
        if (t < K) lam[((size_t)(Nt - 1) * mb + b) * K + t] = l;
    } else if (Nt > 1) load_chunk(Nt - 1, chain_lds);
    __syncthreads();
    int cur = 0;
    for (int s_hi = Nt - 1; s_hi >= 1; s_hi -= steps_per_chunk, cur ^= 1) {
        const int s_lo = chunk_lo(s_hi), ns = s_hi - s_lo + 1;
        if (t >= 64) {
            if (s_lo > 1) load_chunk(s_lo - 1, chain_lds + (size_t)(cur ^ 1) * bufsz);
        } else {
            const float* buf = chain_lds + (size_t)cur * bufsz;
            const int j = t < KC ? t : KC - 1;                 // lanes >= K read zero columns
            for (int q = ns - 1; q >= 0; --q) {
                const float* Jq = buf + q * MS + j;
                float a[4] = {Jq[KC * KC], 0.f, 0.f, 0.f};    // g[s - 1][j]
                float col[KC];
#pragma unroll
                for (int i = 0; i < KC; ++i) col[i] = Jq[i * KC];
#pragma unroll
                for (int i = 0; i < KC; ++i) {
                    const float li = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, l), i));
                    a[i & 3] = fmaf(li, col[i], a[i & 3]);
                }
                l = (a[0] + a[1]) + (a[2] + a[3]);
                if (t < K) lam[((size_t)(s_lo + q - 1) * mb + b) * K + t] = l;
            }
        }
        __syncthreads();
    }
}

constexpr size_t kFwdLds = (size_t)(kMlpFloats + 2 * TB * HS + 4 * TB * KS + 64) * sizeof(float);
constexpr size_t kBwdLds = (size_t)(kMlpFloats + 3 * TB * HS + 10 * TB * KS + 64) * sizeof(float);

int method_id(int method) { return (method >= 0 && method <= 2) ? method : -1; }

}  // namespace

NNS_API size_t nns_ode_mlp_bwd_workspace(int mb) {
    if (mb < 1) return 0;
    return (size_t)((mb + TB - 1) / TB) * 4 * kStageFloats * sizeof(float);
}

NNS_API int nns_ode_mlp_fwd_f32(const float* z0, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                const float* b2, float* out, int mb, int K, int hidden, int Nt, int method, void* stream) {
    if (!z0 || !W0 || !b0 || !W1 || !b1 || !W2 || !b2 || !out || mb < 1 || Nt < 1) return fail(NNS_ERR_INVALID_ARG, "ode_mlp_fwd: bad args");
    if (hidden != H) return fail(NNS_ERR_UNSUPPORTED, "ode_mlp_fwd: hidden width %d (the reference's ODEFunc is fixed at %d)", hidden, H);
    if (K < 1 || K > KP) return fail(NNS_ERR_UNSUPPORTED, "ode_mlp_fwd: K=%d not in [1, %d]", K, KP);
    if (method_id(method) < 0) return fail(NNS_ERR_INVALID_ARG, "ode_mlp_fwd: method %d (0 Euler, 1 RK2, 2 RK4)", method);
    if (int rc = lds_opt_in<ode_mlp_fwd_kernel>((int)kFwdLds, "ode_mlp_fwd")) return rc;
    static const int row_max = [] { const char* e = getenv("NNS_ODE_ROW_MAX"); return e ? atoi(e) : 4096; }();      // 0 forces the MFMA tile kernel (A/B, tests)
    if (mb <= row_max) {
        // one row per workgroup, weights in registers: ~2.6 us per RK4 step whatever the batch, against 14 us for a 16-row MFMA tile
        hipLaunchKernelGGL(ode_mlp_fwd_row_kernel, dim3(mb), dim3(RT), 0, as_stream(stream), z0, W0, b0, W1, b1, W2, b2, out, mb, K, Nt, method);
        return check_launch("ode_mlp_fwd");
    }
    hipLaunchKernelGGL(ode_mlp_fwd_kernel, dim3((mb + TB - 1) / TB), dim3(NT), kFwdLds, as_stream(stream), z0, W0, b0, W1, b1, W2, b2, out, mb, K, Nt, method);
    return check_launch("ode_mlp_fwd");
}

static int ode_mlp_bwd_impl(const char* what, const float* z0, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                            const float* b2, const float* states, const float* grad_out, float* grad_z0, float* gW0, float* gb0,
                            float* gW1, float* gb1, float* gW2, float* gb2, void* work, int mb, int K, int hidden, int Nt, int method, float dt_in,
                            void* stream) {
    const bool all_pg = gW0 && gb0 && gW1 && gb1 && gW2 && gb2, no_pg = !gW0 && !gb0 && !gW1 && !gb1 && !gW2 && !gb2;
    if (!z0 || !W0 || !b0 || !W1 || !b1 || !W2 || !b2 || !states || !grad_out || !grad_z0 || !(all_pg || (no_pg && dt_in > 0.f)) || !work ||
        mb < 1 || Nt < 1)
        return fail(NNS_ERR_INVALID_ARG, "%s: bad args (the six parameter-gradient pointers: all set, or -- independent steps only -- all NULL)", what);
    if (hidden != H) return fail(NNS_ERR_UNSUPPORTED, "%s: hidden width %d (fixed at %d)", what, hidden, H);
    if (K < 1 || K > KP) return fail(NNS_ERR_UNSUPPORTED, "%s: K=%d not in [1, %d]", what, K, KP);
    if (method_id(method) < 0) return fail(NNS_ERR_INVALID_ARG, "%s: method %d", what, method);
    if (int rc = lds_opt_in<ode_mlp_bwd_kernel>((int)kBwdLds, what)) return rc;
    hipStream_t s = as_stream(stream);
    // the parameter gradients are accumulated with atomics: zero them first -- ONE launch for the six buffers (round 4: six memsets before)
    if (all_pg) {
        void* const bufs[6] = {gW0, gb0, gW1, gb1, gW2, gb2};
        const long bytes[6] = {(long)H * K * 4, (long)H * 4, (long)H * H * 4, (long)H * 4, (long)K * H * 4, (long)K * 4};
        const int rc = zero_buffers(bufs, bytes, 6, s);
        if (rc != NNS_OK) return rc;
    }
    hipLaunchKernelGGL(ode_mlp_bwd_kernel, dim3((mb + TB - 1) / TB), dim3(NT), kBwdLds, s, z0, W0, b0, W1, b1, W2, b2, states, grad_out,
                       grad_z0, gW0, gb0, gW1, gb1, gW2, gb2, reinterpret_cast<float*>(work), mb, K, Nt, method, dt_in);
    return check_launch(what);
}

NNS_API int nns_ode_mlp_bwd_f32(const float* z0, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                const float* b2, const float* states, const float* grad_out, float* grad_z0, float* gW0, float* gb0,
                                float* gW1, float* gb1, float* gW2, float* gb2, void* work, int mb, int K, int hidden, int Nt, int method,
                                void* stream) {
    return ode_mlp_bwd_impl("ode_mlp_bwd", z0, W0, b0, W1, b1, W2, b2, states, grad_out, grad_z0, gW0, gb0, gW1, gb1, gW2, gb2, work, mb, K, hidden,
                            Nt, method, 0.f, stream);
}

// Backward of `rows` INDEPENDENT single steps y -> y' of step size dt (the time-parallel adjoint, nns/neural_spectral/anode.py):
// grad_y[r] = (d y'[r] / d y[r])^T grad_out[r], parameter gradients summed over the rows.
NNS_API int nns_ode_mlp_bwd_steps_f32(const float* y, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                      const float* b2, const float* grad_out, float* grad_y, float* gW0, float* gb0, float* gW1, float* gb1,
                                      float* gW2, float* gb2, void* work, int rows, int K, int hidden, double dt, int method, void* stream) {
    if (!(dt > 0)) return fail(NNS_ERR_INVALID_ARG, "ode_mlp_bwd_steps: dt must be > 0");
    return ode_mlp_bwd_impl("ode_mlp_bwd_steps", y, W0, b0, W1, b1, W2, b2, y /* states: unused with one step */, grad_out, grad_y, gW0, gb0, gW1, gb1,
                            gW2, gb2, work, rows, K, hidden, 1, method, (float)dt, stream);
}

NNS_API int nns_ode_adjoint_chain_f32(const float* J, const float* g, float* lam, int Nt, int mb, int K, void* stream) {
    if (!J || !g || !lam || Nt < 1 || mb < 1 || K < 1 || K > 64) return fail(NNS_ERR_INVALID_ARG, "ode_adjoint_chain: bad args (Nt=%d mb=%d K=%d)", Nt, mb, K);
    const int KC = K <= 32 ? 32 : 64;
    int spc = kChainLdsFloats / (KC * KC + KC);
    if (spc > Nt) spc = Nt;
    if (spc < 1) spc = 1;
    const int lds = 2 * spc * (KC * KC + KC) * (int)sizeof(float);
    const int vec4 = (K * K) % 4 == 0 && (reinterpret_cast<uintptr_t>(J) & 15) == 0;
    auto magic = [](unsigned d) { return d == 1 ? 0u : (unsigned)((1ull << 32) / d + 1); };
    const unsigned mK = magic((unsigned)K), mKK = magic((unsigned)(vec4 ? K * K / 4 : K * K));
    auto launch = [&](auto kc) -> int {
        constexpr auto kern = ode_adjoint_chain_kernel<decltype(kc)::value>;
        if (int rc = lds_opt_in<kern>(lds, "ode_adjoint_chain")) return rc;          // lds grows with Nt: one call per increase
        hipLaunchKernelGGL(kern, dim3(mb), dim3(kChainThreads), lds, as_stream(stream), J, g, lam, Nt, mb, K, spc, vec4, mK, mKK);
        return check_launch("ode_adjoint_chain");
    };
    return K <= 32 ? launch(std::integral_constant<int, 32>{}) : launch(std::integral_constant<int, 64>{});
}
