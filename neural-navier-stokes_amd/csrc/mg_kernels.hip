// Multigrid solve of chorin_fd's pressure equation (an option of the build: SURVEY.md section 8 (f) rank 3, "red-black SOR / multigrid").
//
// The equation is the fixed point of the reference's SOR update (src/chorin_fd/simulate.py:186-196) on interior points,
//     dy^2 (p[i+1,j] + p[i-1,j] - 2p) + dx^2 (p[i,j+1] + p[i,j-1] - 2p) = C[i,j],
// with p's boundary ring as Dirichlet data (read, never written).  Every level works in the unscaled form Lap_h u = f, f = C / (dx^2 dy^2);
// the restatement is tests/mg_oracle.py (same hierarchy, transfers, sweep orders, stopping rule and info).
//
//   hierarchy    each axis n -> (n - 1) / 2 + 1 nodes, H = h (n - 1) / (nc - 1), until min(nx, ny) <= 9 (non-nested when n - 1 is odd)
//   transfers    P: per-axis linear interpolation by node coordinate; R = (hx / Hx)(hy / Hy) P^T on the residual r = f - Lap_h u
//   cycle        V(2, 2), red-black Gauss-Seidel (weight 1; colour 0 = (i + j) even); pre: colours 0, 1; post: colours 1, 0
//   coarsest     exact solve of the error equation in the sine basis (at most 31 x 31 interior points)
//   stopping     per grid, on the device, after the cycle in which max|r_k| <= tol max|r_0| or max|r_k| >= 0.9 max|r_(k-1)|
//
// Levels too large for one workgroup's LDS run chip-wide, one launch per half-sweep / transfer, blockIdx.z = grid of the batch; the levels
// that fit (<= 150 KB together) run as ONE launch per cycle, one workgroup per grid, everything in LDS down to the coarsest solve.  Every
// kernel reads its grid's active flag first and returns at once when it is off, so a host can enqueue many cycles without reading anything
// back.  Per-grid max-norms: one atomic max on the IEEE bit pattern per workgroup (order-independent: the results are deterministic).
// No grid-wide barrier, no cooperative launch, no cross-workgroup waiting.  Compiled with -ffp-contract=off (the restatement's rounding).
#include "nns_common.h"
#include <climits>
#include <cmath>

using namespace nns;

namespace {

constexpr int kMgMaxLev = 16;
constexpr int kMgThreads = 256;            // chip-wide kernels
constexpr int kMgTailThreads = 1024;       // the LDS tail: one workgroup per grid
constexpr int kMgStopN = 9;                // coarsen while min(nx, ny) > 9
constexpr int kMgMinN = 5;
constexpr int kMgMaxCoarse = 33;           // nodes per axis of the coarsest level (its exact solve holds dense sine tables in LDS)
constexpr double kMgMaxAspect = 2.0;
constexpr size_t kMgLdsMax = 150 * 1024;

template <typename T> struct BitsOf;
template <> struct BitsOf<float> { using U = unsigned int; };
template <> struct BitsOf<double> { using U = unsigned long long; };

template <typename T>
__device__ __forceinline__ T nanmax(T a, T b) { return (b > a || b != b) ? b : a; }

// Per-level constants: cx = 1 / hx^2 (axis 0), cy = 1 / hy^2 (axis 1), d = 2 cx + 2 cy, id = 1 / d; sxy = (hx / Hx)(hy / Hy) to the next level.
template <typename T>
struct MgK {
    int nlev, tail;
    int nx[kMgMaxLev], ny[kMgMaxLev];
    int lds[kMgMaxLev + 1];              // tail levels: element offset of u_l in LDS (f_l follows it); lds[nlev]: the coarse solve's scratch
    T cx[kMgMaxLev], cy[kMgMaxLev], d[kMgMaxLev], id[kMgMaxLev], sxy[kMgMaxLev];
    T s0, tol;
};

// Per-grid solve state at the front of the workspace (the host reads `active`, the first batch int32 of work).
template <typename T>
struct MgState {
    int* active;
    int* done;
    typename BitsOf<T>::U* rbits;        // max|r| of the cycle being finished, as a bit pattern
    T* r0;
    T* rprev;
};

// ------------------------------------------------------------------------------------------------------------------ point operators
template <typename T>
__device__ __forceinline__ void rb_point(T* u, const T* f, T scale, int ny, T cx, T cy, T id, int c) {
    u[c] = (cx * (u[c + ny] + u[c - ny]) + cy * (u[c + 1] + u[c - 1]) - f[c] * scale) * id;
}

template <typename T>
__device__ __forceinline__ T resid(const T* u, const T* f, T scale, int ny, T cx, T cy, T d, int c) {
    return f[c] * scale - (cx * (u[c + ny] + u[c - ny]) + cy * (u[c + 1] + u[c - 1]) - d * u[c]);
}

// fine node i of an axis with n nodes sits at coarse coordinate i (nc - 1) / (n - 1) = i0 + frac
template <typename T>
__device__ __forceinline__ void axis_pos(int i, int n, int nc, int& i0, T& frac) {
    const int num = i * (nc - 1);
    i0 = num / (n - 1);
    frac = (T)(num - i0 * (n - 1)) / (T)(n - 1);
}

template <typename T>
__device__ __forceinline__ T axis_weight(int i, int n, int nc, int I) {
    int i0;
    T fr;
    axis_pos<T>(i, n, nc, i0, fr);
    return i0 == I ? (T)1 - fr : (i0 == I - 1 ? fr : (T)0);
}

// f_c[I][J] = sxy sum_ij Px[i][I] Py[j][J] r[i][j] over fine interior points (coarse interior I, J)
template <typename T>
__device__ __forceinline__ T restrict_point(const T* uf, const T* ff, T scale, int nxf, int nyf, T cx, T cy, T d, int nxc, int nyc, T sxy, int I, int J) {
    const int ilo = max(1, ((I - 1) * (nxf - 1) + nxc - 2) / (nxc - 1)), ihi = min(nxf - 2, ((I + 1) * (nxf - 1)) / (nxc - 1));
    const int jlo = max(1, ((J - 1) * (nyf - 1) + nyc - 2) / (nyc - 1)), jhi = min(nyf - 2, ((J + 1) * (nyf - 1)) / (nyc - 1));
    T acc = (T)0;
    for (int i = ilo; i <= ihi; ++i) {
        const T wx = axis_weight<T>(i, nxf, nxc, I);
        if (wx == (T)0) continue;
        T row = (T)0;
        for (int j = jlo; j <= jhi; ++j) {
            const T wy = axis_weight<T>(j, nyf, nyc, J);
            if (wy != (T)0) row += wy * resid<T>(uf, ff, scale, nyf, cx, cy, d, i * nyf + j);
        }
        acc += wx * row;
    }
    return sxy * acc;
}

// u_f[i][j] += (P e_c)[i][j] (fine interior i, j; the coarse boundary ring is 0)
template <typename T>
__device__ __forceinline__ void prolong_point(T* uf, int nxf, int nyf, const T* uc, int nxc, int nyc, int i, int j) {
    int i0, j0;
    T fx, fy;
    axis_pos<T>(i, nxf, nxc, i0, fx);
    axis_pos<T>(j, nyf, nyc, j0, fy);
    const T* e = uc + i0 * nyc + j0;                       // i0 <= nxc - 2, j0 <= nyc - 2 for interior fine points
    const T a = ((T)1 - fy) * e[0] + fy * e[1], b = ((T)1 - fy) * e[nyc] + fy * e[nyc + 1];
    uf[i * nyf + j] += ((T)1 - fx) * a + fx * b;
}

template <typename T>
__device__ __forceinline__ void finish_cycle(const MgState<T>& st, int b, T r, T tol, T* info) {
    const int k = ++st.done[b];
    const T r0 = st.r0[b];
    info[2 * b] = (T)k;
    info[2 * b + 1] = r / r0;
    st.active[b] = (r > tol * r0 && r < (T)0.9 * st.rprev[b]) ? 1 : 0;      // NaN stops
    st.rprev[b] = r;
}

template <typename T>
__device__ __forceinline__ T sin_pi_ratio(int a, int m) {                 // sin(pi a / m), argument reduced to [0, 2m)
    return sinpi((T)(a % (2 * m)) / (T)m);
}

// ------------------------------------------------------------------------------------------------------------------ chip-wide kernels
template <typename T>
__global__ __launch_bounds__(kMgThreads) void mg_smooth_kernel(T* __restrict__ u, const T* __restrict__ f, T scale, int nx, int ny, T cx, T cy, T id,
                                                             int colour, const int* __restrict__ active) {
    const int b = blockIdx.z;
    if (!active[b]) return;
    const size_t n = (size_t)nx * ny;
    u += b * n;
    f += b * n;
    const int hw = (ny - 1) / 2, q = blockIdx.x * kMgThreads + threadIdx.x;
    if (q >= hw) return;
    for (int i = blockIdx.y + 1; i <= nx - 2; i += gridDim.y) {
        const int j = 1 + 2 * q + ((i + 1 + colour) & 1);                  // (i + j) % 2 == colour
        if (j <= ny - 2) rb_point<T>(u, f, scale, ny, cx, cy, id, i * ny + j);
    }
}

// residual of level l + restriction to level l + 1, one thread per coarse node; also zeroes the coarse correction u_c
template <typename T>
__global__ __launch_bounds__(kMgThreads) void mg_restrict_kernel(const T* __restrict__ uf, const T* __restrict__ ff, T scale, int nxf, int nyf, T cx, T cy, T d,
                                                               T* __restrict__ uc, T* __restrict__ fc, int nxc, int nyc, T sxy, const int* __restrict__ active) {
    const int b = blockIdx.z;
    if (!active[b]) return;
    const size_t nf = (size_t)nxf * nyf, nc = (size_t)nxc * nyc;
    const int idx = blockIdx.x * kMgThreads + threadIdx.x;
    if (idx >= nxc * nyc) return;
    const int I = idx / nyc, J = idx - I * nyc;
    const bool in = I > 0 && I < nxc - 1 && J > 0 && J < nyc - 1;
    uc[b * nc + idx] = (T)0;
    fc[b * nc + idx] = in ? restrict_point<T>(uf + b * nf, ff + b * nf, scale, nxf, nyf, cx, cy, d, nxc, nyc, sxy, I, J) : (T)0;
}

template <typename T>
__global__ __launch_bounds__(kMgThreads) void mg_prolong_kernel(T* __restrict__ uf, int nxf, int nyf, const T* __restrict__ uc, int nxc, int nyc,
                                                              const int* __restrict__ active) {
    const int b = blockIdx.z;
    if (!active[b]) return;
    const int my = nyf - 2, idx = blockIdx.x * kMgThreads + threadIdx.x;
    if (idx >= (nxf - 2) * my) return;
    const int i = idx / my + 1, j = idx - (i - 1) * my + 1;
    prolong_point<T>(uf + b * (size_t)nxf * nyf, nxf, nyf, uc + b * (size_t)nxc * nyc, nxc, nyc, i, j);
}

// max|r| over the interior of the finest level into st.rbits[b]: one guarded atomic max per workgroup
template <typename T>
__global__ __launch_bounds__(kMgThreads) void mg_norm_kernel(const T* __restrict__ u, const T* __restrict__ f, T scale, int nx, int ny, T cx, T cy, T d,
                                                           MgState<T> st) {
    using U = typename BitsOf<T>::U;
    __shared__ T wave_e[kMgThreads / kWave];
    const int b = blockIdx.z;
    if (!st.active[b]) return;
    const size_t n = (size_t)nx * ny;
    u += b * n;
    f += b * n;
    const int my = ny - 2, m = (nx - 2) * my;
    T e = (T)0;
    for (int idx = blockIdx.x * kMgThreads + threadIdx.x; idx < m; idx += gridDim.x * kMgThreads) {
        const int i = idx / my + 1, j = idx - (i - 1) * my + 1;
        e = nanmax<T>(e, fabs(resid<T>(u, f, scale, ny, cx, cy, d, i * ny + j)));
    }
    for (int off = kWave / 2; off > 0; off >>= 1) e = nanmax<T>(e, __shfl_xor(e, off));
    if ((threadIdx.x & (kWave - 1)) == 0) wave_e[threadIdx.x / kWave] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMgThreads / kWave; ++w) e = nanmax<T>(e, wave_e[w]);
        const U bits = __builtin_bit_cast(U, e);
        if (bits > __hip_atomic_load(&st.rbits[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&st.rbits[b], bits);
    }
}

template <typename T>
__global__ void mg_init_kernel(MgState<T> st, int batch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    st.active[b] = 1;
    st.done[b] = 0;
    st.rbits[b] = 0;
}

// start = 1: max|r_0| has just been measured -> (0, 1); for a zero residual (0, 0) and the grid is off; for a NaN or infinite one (a NaN or
// Inf in C or p) (0, NaN) and the grid is off; start = 0: end of a cycle
template <typename T>
__global__ void mg_finish_kernel(MgState<T> st, T* __restrict__ info, int batch, T tol, int start) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch || !st.active[b]) return;
    const T r = __builtin_bit_cast(T, st.rbits[b]);
    st.rbits[b] = 0;
    if (start) {
        const bool finite = __builtin_isfinite(r);
        st.r0[b] = r;
        st.rprev[b] = r;
        st.active[b] = finite && r > (T)0 ? 1 : 0;
        info[2 * b] = (T)0;
        info[2 * b + 1] = !finite ? (T)__builtin_nan("") : (r > (T)0 ? (T)1 : (T)0);
    } else {
        finish_cycle<T>(st, b, r, tol, info);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the LDS tail
template <typename T>
__device__ __forceinline__ void tail_smooth(T* u, const T* f, T scale, int nx, int ny, T cx, T cy, T id, int colour) {
    const int hw = (ny - 1) / 2, half = (nx - 2) * hw;
    for (int q = threadIdx.x; q < half; q += kMgTailThreads) {
        const int i = q / hw + 1;
        const int j = 1 + 2 * (q - (i - 1) * hw) + ((i + 1 + colour) & 1);
        if (j <= ny - 2) rb_point<T>(u, f, scale, ny, cx, cy, id, i * ny + j);
    }
    __syncthreads();
}

// the coarsest level: e = Lap_h^-1 r (zero boundary) in the sine basis, u += e; w: LDS scratch of mx^2 + my^2 + 2 mx my elements
template <typename T>
__device__ __forceinline__ void tail_coarse(T* u, const T* f, T scale, int nx, int ny, T cx, T cy, T d, T* w) {
    const int mx = nx - 2, my = ny - 2, tid = threadIdx.x;
    T* Sx = w;
    T* Sy = Sx + mx * mx;
    T* W1 = Sy + my * my;
    T* W2 = W1 + mx * my;
    for (int t = tid; t < mx * mx; t += kMgTailThreads) Sx[t] = sin_pi_ratio<T>((t / mx + 1) * (t % mx + 1), nx - 1);
    for (int t = tid; t < my * my; t += kMgTailThreads) Sy[t] = sin_pi_ratio<T>((t / my + 1) * (t % my + 1), ny - 1);
    for (int t = tid; t < mx * my; t += kMgTailThreads) W2[t] = resid<T>(u, f, scale, ny, cx, cy, d, (t / my + 1) * ny + t % my + 1);
    __syncthreads();
    for (int t = tid; t < mx * my; t += kMgTailThreads) {            // W1 = Sx r
        const int k = t / my, j = t % my;
        T s = (T)0;
        for (int i = 0; i < mx; ++i) s += Sx[k * mx + i] * W2[i * my + j];
        W1[t] = s;
    }
    __syncthreads();
    for (int t = tid; t < mx * my; t += kMgTailThreads) {            // W2 = (W1 Sy) / (lx_k + ly_l)
        const int k = t / my, l = t % my;
        T s = (T)0;
        for (int j = 0; j < my; ++j) s += W1[k * my + j] * Sy[l * my + j];
        const T sx = sinpi((T)(k + 1) / (T)(2 * (nx - 1))), sy = sinpi((T)(l + 1) / (T)(2 * (ny - 1)));
        W2[t] = s / ((T)-4 * cx * (sx * sx) + (T)-4 * cy * (sy * sy));
    }
    __syncthreads();
    for (int t = tid; t < mx * my; t += kMgTailThreads) {            // W1 = Sx W2
        const int i = t / my, l = t % my;
        T s = (T)0;
        for (int k = 0; k < mx; ++k) s += Sx[i * mx + k] * W2[k * my + l];
        W1[t] = s;
    }
    __syncthreads();
    const T c = ((T)2 / (T)(nx - 1)) * ((T)2 / (T)(ny - 1));
    for (int t = tid; t < mx * my; t += kMgTailThreads) {            // u += c W1 Sy
        const int i = t / my, j = t % my;
        T s = (T)0;
        for (int l = 0; l < my; ++l) s += W1[i * my + l] * Sy[j * my + l];
        u[(i + 1) * ny + j + 1] += c * s;
    }
    __syncthreads();
}

// One V-cycle of levels tail .. nlev - 1 per workgroup (= grid b): u_g / f_g (scale) are level `tail`'s correction and right-hand side in
// global memory (p and C when tail = 0).  The boundary ring of u_g is never written.  finish (tail = 0): the workgroup also measures
// max|r| of the result and closes the cycle (what mg_norm_kernel + mg_finish_kernel do on the chip-wide path).
template <typename T>
__global__ __launch_bounds__(kMgTailThreads) void mg_tail_kernel(MgK<T> k, T* __restrict__ u_g, const T* __restrict__ f_g, T scale, MgState<T> st,
                                                               T* __restrict__ info, int finish) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mg_smem[];
    __shared__ T red[kMgTailThreads / kWave];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (!st.active[b]) return;
    const int L = k.tail, Lc = k.nlev - 1;
    auto lev = [&](int l) { return reinterpret_cast<T*>(mg_smem) + k.lds[l]; };
    T* scratch = lev(k.nlev);
    const int n = k.nx[L] * k.ny[L];
    u_g += (size_t)b * n;
    f_g += (size_t)b * n;
    for (int c = tid; c < n; c += kMgTailThreads) { lev(L)[c] = u_g[c]; lev(L)[n + c] = f_g[c] * scale; }
    __syncthreads();
    for (int l = L; l < Lc; ++l) {
        const int nx = k.nx[l], ny = k.ny[l];
        T* u = lev(l);
        const T* f = u + nx * ny;
        for (int s = 0; s < 2; ++s) {
            tail_smooth<T>(u, f, (T)1, nx, ny, k.cx[l], k.cy[l], k.id[l], 0);
            tail_smooth<T>(u, f, (T)1, nx, ny, k.cx[l], k.cy[l], k.id[l], 1);
        }
        const int nxc = k.nx[l + 1], nyc = k.ny[l + 1];
        T* uc = lev(l + 1);
        T* fc = uc + nxc * nyc;
        for (int idx = tid; idx < nxc * nyc; idx += kMgTailThreads) {
            const int I = idx / nyc, J = idx - I * nyc;
            const bool in = I > 0 && I < nxc - 1 && J > 0 && J < nyc - 1;
            uc[idx] = (T)0;
            fc[idx] = in ? restrict_point<T>(u, f, (T)1, nx, ny, k.cx[l], k.cy[l], k.d[l], nxc, nyc, k.sxy[l], I, J) : (T)0;
        }
        __syncthreads();
    }
    tail_coarse<T>(lev(Lc), lev(Lc) + k.nx[Lc] * k.ny[Lc], (T)1, k.nx[Lc], k.ny[Lc], k.cx[Lc], k.cy[Lc], k.d[Lc], scratch);
    for (int l = Lc - 1; l >= L; --l) {
        const int nx = k.nx[l], ny = k.ny[l], my = ny - 2;
        T* u = lev(l);
        const T* f = u + nx * ny;
        for (int idx = tid; idx < (nx - 2) * my; idx += kMgTailThreads) {
            const int i = idx / my + 1, j = idx - (i - 1) * my + 1;
            prolong_point<T>(u, nx, ny, lev(l + 1), k.nx[l + 1], k.ny[l + 1], i, j);
        }
        __syncthreads();
        for (int s = 0; s < 2; ++s) {
            tail_smooth<T>(u, f, (T)1, nx, ny, k.cx[l], k.cy[l], k.id[l], 1);
            tail_smooth<T>(u, f, (T)1, nx, ny, k.cx[l], k.cy[l], k.id[l], 0);
        }
    }
    const int nx = k.nx[L], ny = k.ny[L], my = ny - 2;
    T e = (T)0;
    for (int idx = tid; idx < (nx - 2) * my; idx += kMgTailThreads) {
        const int c = (idx / my + 1) * ny + idx % my + 1;
        u_g[c] = lev(L)[c];                                             // interior only
        if (finish) e = nanmax<T>(e, fabs(resid<T>(lev(L), lev(L) + n, (T)1, ny, k.cx[L], k.cy[L], k.d[L], c)));
    }
    if (!finish) return;
    for (int off = kWave / 2; off > 0; off >>= 1) e = nanmax<T>(e, __shfl_xor(e, off));
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = e;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kMgTailThreads / kWave; ++w) e = nanmax<T>(e, red[w]);
        finish_cycle<T>(st, b, e, k.tol, info);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct MgShape {
    int nlev;
    int nx[kMgMaxLev], ny[kMgMaxLev];
};

int mg_shape(int nx, int ny, MgShape& s, const char* what) {
    if (nx < kMgMinN || ny < kMgMinN)
        return fail(NNS_ERR_UNSUPPORTED, "%s: multigrid needs at least %d nodes per axis, got %d x %d", what, kMgMinN, nx, ny);
    if ((long)nx * ny > (long)INT_MAX / 4) return fail(NNS_ERR_UNSUPPORTED, "%s: %d x %d grid too large", what, nx, ny);
    s.nlev = 1;
    s.nx[0] = nx;
    s.ny[0] = ny;
    while (std::min(s.nx[s.nlev - 1], s.ny[s.nlev - 1]) > kMgStopN) {
        if (s.nlev == kMgMaxLev) return fail(NNS_ERR_UNSUPPORTED, "%s: more than %d levels", what, kMgMaxLev);
        s.nx[s.nlev] = (s.nx[s.nlev - 1] - 1) / 2 + 1;
        s.ny[s.nlev] = (s.ny[s.nlev - 1] - 1) / 2 + 1;
        ++s.nlev;
    }
    const int l = s.nlev - 1;
    if (s.nx[l] > kMgMaxCoarse || s.ny[l] > kMgMaxCoarse)
        return fail(NNS_ERR_UNSUPPORTED, "%s: coarsest level %d x %d exceeds %d nodes on an axis", what, s.nx[l], s.ny[l], kMgMaxCoarse);
    return NNS_OK;
}

// LDS of a tail starting at level l (elements): u and f of every level, then the coarse solve's sine tables and two work arrays
size_t tail_lds_elems(const MgShape& s, int l) {
    size_t e = 0;
    for (int m = l; m < s.nlev; ++m) e += 2 * (size_t)s.nx[m] * s.ny[m];
    const size_t mx = s.nx[s.nlev - 1] - 2, my = s.ny[s.nlev - 1] - 2;
    return e + mx * mx + my * my + 2 * mx * my;
}

int tail_level(const MgShape& s, size_t elem) {
    int l = s.nlev - 1;
    while (l > 0 && tail_lds_elems(s, l - 1) * elem <= kMgLdsMax) --l;
    return l;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace: [int active[B]][int done[B]][8-byte rbits[B]][8-byte r0[B]][8-byte rprev[B]], then u_l, f_l [B][n_l] of each chip-wide level l >= 1
size_t state_bytes(int batch) { return align256((size_t)batch * (4 + 4 + 8 + 8 + 8)); }

size_t level_bytes(const MgShape& s, int l, int batch, size_t elem) { return align256((size_t)batch * s.nx[l] * s.ny[l] * elem); }

size_t mg_bytes(const MgShape& s, int batch, size_t elem) {
    size_t b = state_bytes(batch);
    for (int l = 1; l < tail_level(s, elem) + 1 && l < s.nlev; ++l) b += 2 * level_bytes(s, l, batch, elem);
    return b;
}

template <typename T>
MgState<T> state_of(void* work, int batch) {
    unsigned char* w = static_cast<unsigned char*>(work);
    MgState<T> st;
    st.active = reinterpret_cast<int*>(w);
    st.done = reinterpret_cast<int*>(w + 4 * (size_t)batch);
    st.rbits = reinterpret_cast<typename BitsOf<T>::U*>(w + 8 * (size_t)batch);
    st.r0 = reinterpret_cast<T*>(w + 16 * (size_t)batch);
    st.rprev = reinterpret_cast<T*>(w + 24 * (size_t)batch);
    return st;
}

template <typename T>
int mg_solve(T* p, const T* C, T* info, void* work, int batch, int nx, int ny, double dx, double dy, double tol, int cycles, int resume, hipStream_t s) {
    const char* what = "fd_poisson_mg";
    if (!p || !C || !info || !work || !field_args_ok(batch, nx, ny) || cycles < 0 || (resume != 0 && resume != 1) || !(dx > 0) || !(dy > 0) ||
        !(tol >= 0))
        return fail(NNS_ERR_INVALID_ARG, "%s: bad args (p=%p C=%p info=%p work=%p batch=%d nx=%d ny=%d dx=%g dy=%g tol=%g cycles=%d resume=%d)", what,
                    (void*)p, (const void*)C, (void*)info, work, batch, nx, ny, dx, dy, tol, cycles, resume);
    MgShape sh;
    if (int rc = mg_shape(nx, ny, sh, what)) return rc;
    if (batch > 65535) return fail(NNS_ERR_UNSUPPORTED, "%s: batch %d exceeds the launch grid (65535)", what, batch);
    MgK<T> k{};
    k.nlev = sh.nlev;
    k.tail = tail_level(sh, sizeof(T));
    double hx = dx, hy = dy;
    for (int l = 0; l < sh.nlev; ++l) {
        if (std::max(hx / hy, hy / hx) > kMgMaxAspect)
            return fail(NNS_ERR_UNSUPPORTED, "%s: cell aspect ratio %g > %g at level %d (%d x %d)", what, std::max(hx / hy, hy / hx), kMgMaxAspect, l,
                        sh.nx[l], sh.ny[l]);
        const double cx = 1.0 / (hx * hx), cy = 1.0 / (hy * hy), d = 2.0 * cx + 2.0 * cy;
        k.nx[l] = sh.nx[l];
        k.ny[l] = sh.ny[l];
        k.cx[l] = (T)cx; k.cy[l] = (T)cy; k.d[l] = (T)d; k.id[l] = (T)(1.0 / d);
        if (l + 1 < sh.nlev) {
            const double Hx = hx * (sh.nx[l] - 1) / (sh.nx[l + 1] - 1), Hy = hy * (sh.ny[l] - 1) / (sh.ny[l + 1] - 1);
            k.sxy[l] = (T)((hx / Hx) * (hy / Hy));
            hx = Hx;
            hy = Hy;
        }
    }
    for (int l = k.tail, o = 0; l <= sh.nlev; ++l) {
        k.lds[l] = o;
        if (l < sh.nlev) o += 2 * sh.nx[l] * sh.ny[l];
    }
    k.s0 = (T)(1.0 / (dx * dx * dy * dy));
    k.tol = (T)tol;

    const MgState<T> st = state_of<T>(work, batch);
    // level pointers: 0 = (p, C, s0); 1 .. tail in the workspace
    T* u[kMgMaxLev];
    const T* f[kMgMaxLev];
    T sc[kMgMaxLev];
    u[0] = p; f[0] = C; sc[0] = k.s0;
    {
        unsigned char* q = static_cast<unsigned char*>(work) + state_bytes(batch);
        for (int l = 1; l <= k.tail && l < sh.nlev; ++l) {
            u[l] = reinterpret_cast<T*>(q);
            q += level_bytes(sh, l, batch, sizeof(T));
            f[l] = reinterpret_cast<T*>(q);
            q += level_bytes(sh, l, batch, sizeof(T));
            sc[l] = (T)1;
        }
    }
    const size_t lds = tail_lds_elems(sh, k.tail) * sizeof(T);
    if (int rc = lds_opt_in<mg_tail_kernel<T>>((int)kMgLdsMax, what)) return rc;       // the largest size used: one opt-in for every grid
    const dim3 fin_grid((batch + 255) / 256), fin_block(256);
    auto norm = [&]() {
        const int m = (nx - 2) * (ny - 2);
        const int gx = std::max(1, std::min((m + kMgThreads - 1) / kMgThreads, std::max(1, 2048 / batch)));
        hipLaunchKernelGGL(mg_norm_kernel<T>, dim3(gx, 1, batch), dim3(kMgThreads), 0, s, p, C, k.s0, nx, ny, k.cx[0], k.cy[0], k.d[0], st);
    };
    auto smooth = [&](int l, int colour) {
        const int hw = (k.ny[l] - 1) / 2, gx = (hw + kMgThreads - 1) / kMgThreads;
        const int gy = std::min(k.nx[l] - 2, std::max(1, 2048 / (gx * batch)));
        hipLaunchKernelGGL(mg_smooth_kernel<T>, dim3(gx, gy, batch), dim3(kMgThreads), 0, s, u[l], f[l], sc[l], k.nx[l], k.ny[l], k.cx[l], k.cy[l],
                           k.id[l], colour, st.active);
    };
    if (!resume) {
        hipLaunchKernelGGL(mg_init_kernel<T>, fin_grid, fin_block, 0, s, st, batch);
        norm();
        hipLaunchKernelGGL(mg_finish_kernel<T>, fin_grid, fin_block, 0, s, st, info, batch, k.tol, 1);
    }
    for (int c = 0; c < cycles; ++c) {
        for (int l = 0; l < k.tail; ++l) {
            for (int sw = 0; sw < 2; ++sw) { smooth(l, 0); smooth(l, 1); }
            const int nc = k.nx[l + 1] * k.ny[l + 1];
            hipLaunchKernelGGL(mg_restrict_kernel<T>, dim3((nc + kMgThreads - 1) / kMgThreads, 1, batch), dim3(kMgThreads), 0, s, u[l], f[l], sc[l], k.nx[l],
                               k.ny[l], k.cx[l], k.cy[l], k.d[l], u[l + 1], const_cast<T*>(f[l + 1]), k.nx[l + 1], k.ny[l + 1], k.sxy[l], st.active);
        }
        hipLaunchKernelGGL(mg_tail_kernel<T>, dim3(batch), dim3(kMgTailThreads), lds, s, k, u[k.tail], f[k.tail], sc[k.tail], st, info, k.tail == 0 ? 1 : 0);
        for (int l = k.tail - 1; l >= 0; --l) {
            const int m = (k.nx[l] - 2) * (k.ny[l] - 2);
            hipLaunchKernelGGL(mg_prolong_kernel<T>, dim3((m + kMgThreads - 1) / kMgThreads, 1, batch), dim3(kMgThreads), 0, s, u[l], k.nx[l], k.ny[l],
                               u[l + 1], k.nx[l + 1], k.ny[l + 1], st.active);
            for (int sw = 0; sw < 2; ++sw) { smooth(l, 1); smooth(l, 0); }
        }
        if (k.tail > 0) {
            norm();
            hipLaunchKernelGGL(mg_finish_kernel<T>, fin_grid, fin_block, 0, s, st, info, batch, k.tol, 0);
        }
    }
    return check_launch(what);
}

}  // namespace

NNS_API int nns_fd_poisson_mg_workspace(int batch, int nx, int ny, int elem_size, size_t* bytes) {
    if (!bytes || batch < 1 || nx < 3 || ny < 3 || (elem_size != 4 && elem_size != 8))
        return fail(NNS_ERR_INVALID_ARG, "fd_poisson_mg_workspace: bad args (bytes=%p batch=%d nx=%d ny=%d elem_size=%d)", (void*)bytes, batch, nx, ny,
                    elem_size);
    MgShape sh;
    if (int rc = mg_shape(nx, ny, sh, "fd_poisson_mg_workspace")) return rc;
    *bytes = mg_bytes(sh, batch, (size_t)elem_size);
    return NNS_OK;
}
NNS_API int nns_fd_poisson_mg_f32(float* p, const float* C, float* info, void* work, int batch, int nx, int ny, double dx, double dy, double tol,
                                  int cycles, int resume, void* stream) {
    return mg_solve<float>(p, C, info, work, batch, nx, ny, dx, dy, tol, cycles, resume, as_stream(stream));
}
NNS_API int nns_fd_poisson_mg_f64(double* p, const double* C, double* info, void* work, int batch, int nx, int ny, double dx, double dy, double tol,
                                  int cycles, int resume, void* stream) {
    return mg_solve<double>(p, C, info, work, batch, nx, ny, dx, dy, tol, cycles, resume, as_stream(stream));
}
