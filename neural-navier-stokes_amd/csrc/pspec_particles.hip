// Lagrangian tracers of the periodic solver (include/nns.h: nns_spec_ns_particle_*; restatement: tests/pspec_particles_oracle.py): periodic
// tensor-product B-splines of order 4 (cubic, 4 x 4 nodes) or 6 (quintic, 6 x 6 nodes) of u, v, w, theta, and one Runge-Kutta stage of the
// particles' positions.  A translation unit of its own: it reads the solver's compact spectra (pspec_device.h names the layout's helpers) and
// calls the public nns_spec_irfft2_f32; nothing of pspec_kernels.hip is compiled here.
//   coefs:  one pointwise kernel expands w^ (and theta^) to the half spectra of the chosen fields divided by the splines' symbol
//           beta_x(2 pi m_x / nx) beta_y(2 pi m_y / ny) -- the exact prefilter, beta >= 0.5 (order 4) / 0.325 (order 6) inside the 2/3 band --
//           then nns_spec_irfft2_f32 over nfields B grids gives the coefficient images, float32 [nfields][B][nx][ny].
//   sample / stage:  one lane per particle, templated on the order.  Cell i = floor(x / hx) and offset t = x / hx - i in float64, the 4 or 6
//           weights per axis in float64 and rounded once to float32 registers; nodes i-1 .. i+2 (i-2 .. i+3) modulo n.  The value is
//               sum_a wx[a] (sum_c wy[c] C[i+a][j+c]),
//           the inner sum an fmaf chain over c ascending from 0, the outer an fmaf chain over a ascending from 0: a fixed order, no atomics,
//           no cross-lane reduction, so a particle's result depends only on its own position and its grid's coefficients.  The access is a
//           random gather of 4- or 6-float runs along y into nx ny 4 bytes per grid and field, served by L2 and the Infinity Cache; a run
//           that does not wrap around the row's end is read by one or two wide loads (4-byte aligned), else node by node.
//           Every node index is masked with n - 1 (n a power of two), so no position -- huge, infinite or nan -- reads outside its grid.
#include "pspec_device.h"

#include <cmath>

namespace {

constexpr int kPT = 256;                   // lanes (particles) per workgroup

inline int kept_y(int ny) { return (ny - 1) / 3 + 1; }
inline unsigned pw_grid(long n) { return capped_grid((n + 255) / 256, 4096); }
inline int popcount4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }

// the symbol of the order's B-spline at theta = 2 pi m / n, cos by cospi of the exact ratio
__device__ __forceinline__ double ps_beta(int order, int m, int n) {
    const double c1 = cospi(2.0 * (double)m / (double)n);
    if (order == 4) return (2.0 + c1) / 3.0;
    const double c2 = cospi(4.0 * (double)m / (double)n);
    return (66.0 + 52.0 * c1 + 2.0 * c2) / 120.0;
}

// out[f][b][i][j] (rfft2 layout, nh = ny / 2 + 1) = the spectrum of the f-th chosen field / (beta_x beta_y); fields by ascending bit:
// 0 u, 1 v (from w^ as ps_derivs_kernel makes them, the means in the (0, 0) coefficient), 2 w, 3 theta.  Zero beyond j < my1.
__global__ void ps_particle_spectra_kernel(const float2* __restrict__ W, const float2* __restrict__ T, const float* __restrict__ mean,
                                           float2* __restrict__ out, int mask, int order, int batch, int nx, int ny, int my1, float kx1,
                                           float ky1) {
    const long nh = ny / 2 + 1, per = (long)batch * nx * nh;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < per; q += (long)gridDim.x * blockDim.x) {
        const int j = (int)(q % nh), i = (int)((q / nh) % nx);
        const long b = q / ((long)nx * nh);
        const int mx = i < nx / 2 ? i : i - nx;
        cf u = {0.f, 0.f}, v = u, w = u, th = u;
        if (j < my1) {
            const size_t at = ((size_t)b * my1 + j) * nx + i;
            const float2 w2 = W[at];
            const float kx = kx1 * (float)mx, ky = ky1 * (float)j, k2 = kx * kx + ky * ky;
            const cf psi = k2 > 0.f ? cf{w2.x / k2, w2.y / k2} : cf{0.f, 0.f};
            u = imul(ky, psi);
            v = imul(-kx, psi);
            w = {w2.x, w2.y};
            if (i == 0 && j == 0) {
                const float n = (float)nx * (float)ny;
                u = {mean[2 * b] * n, 0.f}; v = {mean[2 * b + 1] * n, 0.f};
            }
            if (mask & 8) { const float2 t2 = T[at]; th = {t2.x, t2.y}; }
            const float r = (float)(1.0 / (ps_beta(order, mx, nx) * ps_beta(order, j, ny)));
            u = {u.x * r, u.y * r}; v = {v.x * r, v.y * r}; w = {w.x * r, w.y * r}; th = {th.x * r, th.y * r};
        }
        const cf f[4] = {u, v, w, th};
        int slot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (mask & (1 << k)) { out[slot * per + q] = make_float2(f[k].x, f[k].y); ++slot; }
    }
}

// The ORDER weights of offset t in [0, 1], node a = 0 .. ORDER - 1 standing for i - (ORDER / 2 - 1) + a
template <int ORDER>
__device__ __forceinline__ void ps_spline_weights(double t, float (&w)[ORDER]) {
    if constexpr (ORDER == 4) {
        const double s = 1.0 - t, t2 = t * t, t3 = t2 * t;
        w[0] = (float)(s * s * s / 6.0);
        w[1] = (float)((3.0 * t3 - 6.0 * t2 + 4.0) / 6.0);
        w[2] = (float)((-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0);
        w[3] = (float)(t3 / 6.0);
    } else {
        // B5(t - j), j = a - 2: with t in [0, 1] the distance |t - j| of node a lies in a piece known in advance -- a = 0, 5: [2, 3];
        // a = 1, 4: [1, 2]; a = 2, 3: [0, 1]
        const auto inner = [](double x) { const double x2 = x * x, x4 = x2 * x2; return (66.0 - 60.0 * x2 + 30.0 * x4 - 10.0 * x4 * x) / 120.0; };
        const auto middle = [](double x) {
            const double x2 = x * x, x3 = x2 * x, x4 = x2 * x2;
            return (51.0 + 75.0 * x - 210.0 * x2 + 150.0 * x3 - 45.0 * x4 + 5.0 * x4 * x) / 120.0;
        };
        const auto outer = [](double r) { const double r2 = r * r; return r2 * r2 * r / 120.0; };      // r = 3 - |x|
        w[0] = (float)outer(1.0 - t);
        w[1] = (float)middle(t + 1.0);
        w[2] = (float)inner(t);
        w[3] = (float)inner(1.0 - t);
        w[4] = (float)middle(2.0 - t);
        w[5] = (float)outer(t);
    }
}

// cell and offset of coordinate x on an axis of n nodes of spacing h: first node (i - (ORDER / 2 - 1)) mod n in [0, n), weights of t
template <int ORDER>
__device__ __forceinline__ int ps_locate(double x, double h, int n, float (&w)[ORDER]) {
    const double s = x / h, fl = floor(s);
    ps_spline_weights<ORDER>(s - fl, w);
    const double m = fl - (double)n * floor(fl / (double)n);      // exact: n is a power of two
    return ((int)m - (ORDER / 2 - 1)) & (n - 1);                 // the mask also bounds what an infinite or nan x gives
}

// ORDER floats that lie side by side in a row, as one 4-byte aligned object: the compiler loads it with one or two wide instructions
template <int ORDER>
struct __attribute__((packed, aligned(4))) PsRun { float v[ORDER]; };

// RUN: the ORDER y-nodes j0 .. j0 + ORDER - 1 do not wrap around the row's end, so each x-node's run is read as a PsRun; else node by node,
// each index masked.  The same sums in the same order either way.
template <int ORDER, bool RUN>
__device__ __forceinline__ float ps_spline_sum(const float* __restrict__ C, int i0, int j0, int nx, int ny, const float (&wx)[ORDER],
                                               const float (&wy)[ORDER]) {
    float val = 0.f;
#pragma unroll
    for (int a = 0; a < ORDER; ++a) {
        const float* row = C + (size_t)((i0 + a) & (nx - 1)) * ny;
        float r = 0.f;
        if constexpr (RUN) {
            const PsRun<ORDER> run = *reinterpret_cast<const PsRun<ORDER>*>(row + j0);
#pragma unroll
            for (int c = 0; c < ORDER; ++c) r = fmaf(wy[c], run.v[c], r);
        } else {
#pragma unroll
            for (int c = 0; c < ORDER; ++c) r = fmaf(wy[c], row[(j0 + c) & (ny - 1)], r);
        }
        val = fmaf(wx[a], r, val);
    }
    return val;
}

template <int ORDER>
__device__ __forceinline__ float ps_spline_value(const float* __restrict__ C, int i0, int j0, int nx, int ny, const float (&wx)[ORDER],
                                                 const float (&wy)[ORDER]) {
    return j0 + ORDER <= ny ? ps_spline_sum<ORDER, true>(C, i0, j0, nx, ny, wx, wy) : ps_spline_sum<ORDER, false>(C, i0, j0, nx, ny, wx, wy);
}

struct PsBox { int batch, npart, nx, ny; double hx, hy; };

// out[b][p][f] = the spline of coefficient image f at pos[b][p]
template <int ORDER>
__global__ __launch_bounds__(kPT) void ps_particle_sample_kernel(const float* __restrict__ coef, const double* __restrict__ pos,
                                                                 float* __restrict__ out, int nfields, PsBox g) {
    const long total = (long)g.batch * g.npart;
    const long q = blockIdx.x * (long)kPT + threadIdx.x;
    if (q >= total) return;
    const long b = q / g.npart;
    float wx[ORDER], wy[ORDER];
    const int i0 = ps_locate<ORDER>(pos[2 * q], g.hx, g.nx, wx), j0 = ps_locate<ORDER>(pos[2 * q + 1], g.hy, g.ny, wy);
    const size_t image = (size_t)g.nx * g.ny;
    for (int f = 0; f < nfields; ++f)
        out[q * nfields + f] = ps_spline_value<ORDER>(coef + ((size_t)f * g.batch + b) * image, i0, j0, g.nx, g.ny, wx, wy);
}

// One Runge-Kutta stage: k = (u, v)(pos_in) in float32, promoted; s = (FIRST ? 0 : acc) + wk k; CLOSING: pos_out = pos0 + c s (acc is
// not written), else acc = s and pos_out = pos0 + a k.  Every product-sum is one float64 fma.  A lane reads all of its own particle
// before it writes any of it, so pos_in may alias pos0 or pos_out, and pos_out may alias pos0.
template <int ORDER, bool FIRST, bool CLOSING>
__global__ __launch_bounds__(kPT) void ps_particle_stage_kernel(const float* __restrict__ coef, const double* pos0, const double* pos_in,
                                                                double* pos_out, double* acc, double a, double wk, double c, PsBox g) {
    const long total = (long)g.batch * g.npart;
    const long q = blockIdx.x * (long)kPT + threadIdx.x;
    if (q >= total) return;
    const long b = q / g.npart;
    float wx[ORDER], wy[ORDER];
    const int i0 = ps_locate<ORDER>(pos_in[2 * q], g.hx, g.nx, wx), j0 = ps_locate<ORDER>(pos_in[2 * q + 1], g.hy, g.ny, wy);
    const size_t image = (size_t)g.nx * g.ny;
    const double ku = (double)ps_spline_value<ORDER>(coef + (size_t)b * image, i0, j0, g.nx, g.ny, wx, wy);
    const double kv = (double)ps_spline_value<ORDER>(coef + ((size_t)g.batch + b) * image, i0, j0, g.nx, g.ny, wx, wy);
    const double x0 = pos0[2 * q], y0 = pos0[2 * q + 1];
    const double sx = FIRST ? wk * ku : fma(wk, ku, acc[2 * q]), sy = FIRST ? wk * kv : fma(wk, kv, acc[2 * q + 1]);
    if constexpr (CLOSING) {
        pos_out[2 * q] = fma(c, sx, x0);
        pos_out[2 * q + 1] = fma(c, sy, y0);
    } else {
        acc[2 * q] = sx;
        acc[2 * q + 1] = sy;
        pos_out[2 * q] = fma(a, ku, x0);
        pos_out[2 * q + 1] = fma(a, kv, y0);
    }
}

size_t particle_work_bytes(int batch, int nfields, int nx, int ny) { return (size_t)nfields * batch * nx * (ny / 2 + 1) * 2 * sizeof(float); }

// what the three calls check after their own pointers: particles, order, [fields,] the box, the axes
int check_particles(const char* who, int batch, long npart) {
    if (npart < 1 || (long)batch * npart >= (1L << 31))
        return fail(NNS_ERR_INVALID_ARG, "%s: npart = %ld must be >= 1 and batch npart < 2^31", who, npart);
    return NNS_OK;
}
int check_order(const char* who, int order) {
    if (order != 4 && order != 6) return fail(NNS_ERR_INVALID_ARG, "%s: order = %d must be 4 (cubic) or 6 (quintic)", who, order);
    return NNS_OK;
}
int check_particle_box(const char* who, int nx, int ny, double Lx, double Ly) {
    if (!(Lx > 0) || !(Ly > 0) || !std::isfinite(Lx) || !std::isfinite(Ly))
        return fail(NNS_ERR_INVALID_ARG, "%s: Lx = %g, Ly = %g must be positive and finite", who, Lx, Ly);
    if (!pow2_in_range(nx) || !pow2_in_range(ny))
        return fail(NNS_ERR_UNSUPPORTED, "%s: nx = %d, ny = %d: each axis must be a power of two in [64, 1024]", who, nx, ny);
    return NNS_OK;
}

}  // namespace

NNS_API int nns_spec_ns_particle_workspace(int batch, int nfields, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_particle_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (nfields < 1 || nfields > 4) return fail(NNS_ERR_INVALID_ARG, "spec_ns_particle_workspace: nfields = %d must be in [1, 4]", nfields);
    if (!pow2_in_range(nx) || !pow2_in_range(ny))
        return fail(NNS_ERR_UNSUPPORTED, "spec_ns_particle_workspace: nx = %d, ny = %d: each axis must be a power of two in [64, 1024]", nx, ny);
    *bytes = particle_work_bytes(batch, nfields, nx, ny);
    return NNS_OK;
}

NNS_API int nns_spec_ns_particle_coefs_f32(const float* what, const float* that, const float* mean, float* coef, int fields, int order,
                                           void* work, size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, void* stream) {
    const char* who = "spec_ns_particle_coefs";
    if (!what || !mean || !coef || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (int rc = check_order(who, order)) return rc;
    if (fields < 1 || fields > 15) return fail(NNS_ERR_INVALID_ARG, "%s: fields = %d must be a non-empty mask of bits 0 u, 1 v, 2 w, 3 theta", who, fields);
    if ((fields & 8) && !that) return fail(NNS_ERR_INVALID_ARG, "%s: the field mask asks for theta (bit 3) and that is NULL", who);
    if (int rc = check_particle_box(who, nx, ny, Lx, Ly)) return rc;
    const int nfields = popcount4(fields);
    const size_t need = particle_work_bytes(batch, nfields, nx, ny);
    if (work_bytes_ < need)
        return fail(NNS_ERR_WORKSPACE, "%s: workspace of %zu bytes, nns_spec_ns_particle_workspace asks for %zu", who, work_bytes_, need);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ps_particle_spectra_kernel, dim3(pw_grid((long)batch * nx * (ny / 2 + 1))), dim3(256), 0, s,
                       reinterpret_cast<const float2*>(what), reinterpret_cast<const float2*>(that), mean, reinterpret_cast<float2*>(work),
                       fields, order, batch, nx, ny, kept_y(ny), (float)(2.0 * M_PI / Lx), (float)(2.0 * M_PI / Ly));
    if (int rc = check_launch(who)) return rc;
    return nns_spec_irfft2_f32(static_cast<float*>(work), coef, nfields * batch, nx, ny, stream);
}

NNS_API int nns_spec_ns_particle_sample_f32(const float* coef, const double* pos, float* out, int nfields, int order, int batch, long npart,
                                            int nx, int ny, double Lx, double Ly, void* stream) {
    const char* who = "spec_ns_particle_sample";
    if (!coef || !pos || !out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (int rc = check_particles(who, batch, npart)) return rc;
    if (int rc = check_order(who, order)) return rc;
    if (nfields < 1 || nfields > 4) return fail(NNS_ERR_INVALID_ARG, "%s: nfields = %d must be in [1, 4]", who, nfields);
    if (int rc = check_particle_box(who, nx, ny, Lx, Ly)) return rc;
    const PsBox g{batch, (int)npart, nx, ny, Lx / nx, Ly / ny};
    const dim3 grid((unsigned)(((long)batch * npart + kPT - 1) / kPT));
    if (order == 4) hipLaunchKernelGGL(ps_particle_sample_kernel<4>, grid, dim3(kPT), 0, as_stream(stream), coef, pos, out, nfields, g);
    else hipLaunchKernelGGL(ps_particle_sample_kernel<6>, grid, dim3(kPT), 0, as_stream(stream), coef, pos, out, nfields, g);
    return check_launch(who);
}

namespace {
template <int ORDER>
void launch_stage(int first, int closing, dim3 grid, hipStream_t s, const float* coef, const double* pos0, const double* pos_in, double* pos_out,
                  double* acc, double a, double wk, double c, const PsBox& g) {
    if (first && closing) hipLaunchKernelGGL((ps_particle_stage_kernel<ORDER, true, true>), grid, dim3(kPT), 0, s, coef, pos0, pos_in, pos_out, acc, a, wk, c, g);
    else if (first) hipLaunchKernelGGL((ps_particle_stage_kernel<ORDER, true, false>), grid, dim3(kPT), 0, s, coef, pos0, pos_in, pos_out, acc, a, wk, c, g);
    else if (closing) hipLaunchKernelGGL((ps_particle_stage_kernel<ORDER, false, true>), grid, dim3(kPT), 0, s, coef, pos0, pos_in, pos_out, acc, a, wk, c, g);
    else hipLaunchKernelGGL((ps_particle_stage_kernel<ORDER, false, false>), grid, dim3(kPT), 0, s, coef, pos0, pos_in, pos_out, acc, a, wk, c, g);
}
}  // namespace

NNS_API int nns_spec_ns_particle_stage_f32(const float* coef, const double* pos0, const double* pos_in, double* pos_out, double* acc, double a,
                                           double wk, double c, int first, int closing, int order, int batch, long npart, int nx, int ny,
                                           double Lx, double Ly, void* stream) {
    const char* who = "spec_ns_particle_stage";
    if (!coef || !pos0 || !pos_in || !pos_out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (!acc && !(first && closing)) return fail(NNS_ERR_INVALID_ARG, "%s: acc is NULL and the stage is not both first and closing", who);
    if (pos_out == pos0 && !closing) return fail(NNS_ERR_INVALID_ARG, "%s: pos_out may alias pos0 only in the closing stage", who);
    if (int rc = check_particles(who, batch, npart)) return rc;
    if (int rc = check_order(who, order)) return rc;
    if (!std::isfinite(a) || !std::isfinite(wk) || !std::isfinite(c)) return fail(NNS_ERR_INVALID_ARG, "%s: a = %g, wk = %g, c = %g must be finite", who, a, wk, c);
    if (int rc = check_particle_box(who, nx, ny, Lx, Ly)) return rc;
    const PsBox g{batch, (int)npart, nx, ny, Lx / nx, Ly / ny};
    const dim3 grid((unsigned)(((long)batch * npart + kPT - 1) / kPT));
    if (order == 4) launch_stage<4>(first, closing, grid, as_stream(stream), coef, pos0, pos_in, pos_out, acc, a, wk, c, g);
    else launch_stage<6>(first, closing, grid, as_stream(stream), coef, pos0, pos_in, pos_out, acc, a, wk, c, g);
    return check_launch(who);
}

// ---------------------------------------------------------------------------------------------------- reverse mode of the sampling
// (include/nns.h: nns_spec_ns_particle_cells_i32, _spread_f32, _sample_grad_f32, _coefs_adjoint_f32; restatement:
// tests/pspec_particles_adjoint_oracle.py.)
//   cells:   key[b][p] = (b nx + ci) ny + cj, (ci, cj) the wrapped cell of ps_locate (the same float64 floor, the same mask).  The caller sorts
//            the keys (stable: the particles of a cell stay in ascending index) and takes the cells' first slots, start[cells + 1].
//   spread:  the transpose of the gather as a GATHER over the sorted slots, no atomics.  A staging pass (one lane per slot) writes a record
//            (wx[ORDER], wy[ORDER], cot[4]) of kRec<ORDER> floats per slot: a particle's float64 weights are made once, and the node pass
//            reads records that lie in slot order.  The node pass has one lane per node (i, j): the ORDER x ORDER cells whose stencil covers
//            it are ci = i - a + ORDER / 2 - 1, cj = j - c + ORDER / 2 - 1 (masked); a ascending, then c ascending, then the cell's slots
//            ascending; wx[a] wy[c] one float32 multiply, every term one float64 fma into one accumulator per field, rounded once on store.
//            Every node is written.  The trip count of the slot loop differs between the lanes of a wave (a wave runs its fullest cell's);
//            lanes along j read neighbouring cells, whose slots are neighbours too.
//   grad:    the gather of sample with the weights' derivatives on one axis, the same chains: both sums share their loads.
//   coefs adjoint:  nns_spec_rfft2_f32 of the cotangent images, then one pointwise kernel: the forward's multipliers conjugated, the band mask.
namespace {

template <int ORDER> constexpr int kRec = 2 * ORDER + 4;          // floats per record: 48 or 64 bytes, the cotangents 16-byte aligned

// d w[a] / d t of ps_spline_weights, piece by piece
template <int ORDER>
__device__ __forceinline__ void ps_spline_dweights(double t, float (&w)[ORDER]) {
    if constexpr (ORDER == 4) {
        const double s = 1.0 - t, t2 = t * t;
        w[0] = (float)(-s * s / 2.0);
        w[1] = (float)((3.0 * t2 - 4.0 * t) / 2.0);
        w[2] = (float)((-3.0 * t2 + 2.0 * t + 1.0) / 2.0);
        w[3] = (float)(t2 / 2.0);
    } else {
        const auto inner = [](double x) { const double x2 = x * x; return (-120.0 * x + 120.0 * x2 * x - 50.0 * x2 * x2) / 120.0; };
        const auto middle = [](double x) {
            const double x2 = x * x;
            return (75.0 - 420.0 * x + 450.0 * x2 - 180.0 * x2 * x + 25.0 * x2 * x2) / 120.0;
        };
        const auto outer = [](double r) { const double r2 = r * r; return r2 * r2 / 24.0; };            // r = 3 - |x|
        w[0] = (float)(-outer(1.0 - t));
        w[1] = (float)middle(t + 1.0);
        w[2] = (float)inner(t);
        w[3] = (float)(-inner(1.0 - t));
        w[4] = (float)(-middle(2.0 - t));
        w[5] = (float)outer(t);
    }
}

// ps_locate with the derivative weights of the same offset beside the weights
template <int ORDER>
__device__ __forceinline__ int ps_locate_grad(double x, double h, int n, float (&w)[ORDER], float (&dw)[ORDER]) {
    const double s = x / h;
    ps_spline_dweights<ORDER>(s - floor(s), dw);
    return ps_locate<ORDER>(x, h, n, w);
}

// the wrapped cell of ps_locate alone: its first node of order 4 is one node before the cell (the weights are not used)
__device__ __forceinline__ int ps_cell(double x, double h, int n) {
    float w[4];
    return (ps_locate<4>(x, h, n, w) + 1) & (n - 1);
}

__global__ __launch_bounds__(kPT) void ps_particle_cells_kernel(const double* __restrict__ pos, int* __restrict__ key, PsBox g) {
    const long total = (long)g.batch * g.npart;
    const long q = blockIdx.x * (long)kPT + threadIdx.x;
    if (q >= total) return;
    const int b = (int)(q / g.npart);
    key[q] = (b * g.nx + ps_cell(pos[2 * q], g.hx, g.nx)) * g.ny + ps_cell(pos[2 * q + 1], g.hy, g.ny);
}

// ps_spline_sum with a second sum beside it: gx = sum_a dwx[a] (sum_c wy[c] C), gy = sum_a wx[a] (sum_c dwy[c] C), the chains in its order
template <int ORDER, bool RUN>
__device__ __forceinline__ void ps_spline_grad(const float* __restrict__ C, int i0, int j0, int nx, int ny, const float (&wx)[ORDER],
                                               const float (&wy)[ORDER], const float (&dwx)[ORDER], const float (&dwy)[ORDER], float& gx,
                                               float& gy) {
    gx = 0.f;
    gy = 0.f;
#pragma unroll
    for (int a = 0; a < ORDER; ++a) {
        const float* row = C + (size_t)((i0 + a) & (nx - 1)) * ny;
        float r = 0.f, rd = 0.f;
        if constexpr (RUN) {
            const PsRun<ORDER> run = *reinterpret_cast<const PsRun<ORDER>*>(row + j0);
#pragma unroll
            for (int c = 0; c < ORDER; ++c) { r = fmaf(wy[c], run.v[c], r); rd = fmaf(dwy[c], run.v[c], rd); }
        } else {
#pragma unroll
            for (int c = 0; c < ORDER; ++c) {
                const float v = row[(j0 + c) & (ny - 1)];
                r = fmaf(wy[c], v, r);
                rd = fmaf(dwy[c], v, rd);
            }
        }
        gx = fmaf(dwx[a], r, gx);
        gy = fmaf(wx[a], rd, gy);
    }
}

// grad[b][p][f] = (d/dx, d/dy) of the spline of coefficient image f at pos[b][p]: the sums in float32, the division by h in float64
template <int ORDER>
__global__ __launch_bounds__(kPT) void ps_particle_sample_grad_kernel(const float* __restrict__ coef, const double* __restrict__ pos,
                                                                      float* __restrict__ grad, int nfields, PsBox g) {
    const long total = (long)g.batch * g.npart;
    const long q = blockIdx.x * (long)kPT + threadIdx.x;
    if (q >= total) return;
    const long b = q / g.npart;
    float wx[ORDER], wy[ORDER], dwx[ORDER], dwy[ORDER];
    const int i0 = ps_locate_grad<ORDER>(pos[2 * q], g.hx, g.nx, wx, dwx), j0 = ps_locate_grad<ORDER>(pos[2 * q + 1], g.hy, g.ny, wy, dwy);
    const size_t image = (size_t)g.nx * g.ny;
    for (int f = 0; f < nfields; ++f) {
        const float* C = coef + ((size_t)f * g.batch + b) * image;
        float gx, gy;
        if (j0 + ORDER <= g.ny) ps_spline_grad<ORDER, true>(C, i0, j0, g.nx, g.ny, wx, wy, dwx, dwy, gx, gy);
        else ps_spline_grad<ORDER, false>(C, i0, j0, g.nx, g.ny, wx, wy, dwx, dwy, gx, gy);
        reinterpret_cast<float2*>(grad)[q * nfields + f] = make_float2((float)((double)gx / g.hx), (float)((double)gy / g.hy));
    }
}

// Staging pass of the spread: slot s of the sorted order holds particle perm[s] (an index into [batch][npart]); its record is the forward's
// weights and its cotangents, the unused ones zero.  A perm entry outside [0, batch npart) gives a record of zeros: nothing is read for it.
template <int ORDER>
__global__ __launch_bounds__(kPT) void ps_particle_spread_stage_kernel(const float* __restrict__ cot, const double* __restrict__ pos,
                                                                       const long long* __restrict__ perm, float* __restrict__ rec,
                                                                       int nfields, PsBox g) {
    const long total = (long)g.batch * g.npart;
    const long s = blockIdx.x * (long)kPT + threadIdx.x;
    if (s >= total) return;
    const long long p = perm[s];
    float w[2 * ORDER + 4];
#pragma unroll
    for (int k = 0; k < 2 * ORDER + 4; ++k) w[k] = 0.f;
    if (p >= 0 && p < total) {
        float wx[ORDER], wy[ORDER];
        ps_locate<ORDER>(pos[2 * p], g.hx, g.nx, wx);
        ps_locate<ORDER>(pos[2 * p + 1], g.hy, g.ny, wy);
#pragma unroll
        for (int k = 0; k < ORDER; ++k) { w[k] = wx[k]; w[ORDER + k] = wy[k]; }
#pragma unroll
        for (int f = 0; f < 4; ++f)
            if (f < nfields) w[2 * ORDER + f] = cot[p * nfields + f];
    }
    float4* o = reinterpret_cast<float4*>(rec + (size_t)s * kRec<ORDER>);
#pragma unroll
    for (int k = 0; k < kRec<ORDER> / 4; ++k) o[k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// Node pass of the spread: cbar[f][b][i][j] <- the sum over the particles whose stencil covers the node.  start is clamped to the slots
// that exist, so a wrong table reads no record outside the workspace.
template <int ORDER, int NF>
__global__ __launch_bounds__(kPT) void ps_particle_spread_node_kernel(const float* __restrict__ rec, const int* __restrict__ start,
                                                                      float* __restrict__ cbar, PsBox g) {
    const long nodes = (long)g.batch * g.nx * g.ny, total = (long)g.batch * g.npart;
    const long q = blockIdx.x * (long)kPT + threadIdx.x;
    if (q >= nodes) return;
    const int j = (int)(q & (g.ny - 1)), i = (int)((q / g.ny) & (g.nx - 1));
    const long row0 = (q / g.ny - i);                      // b nx
    double acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = 0.0;
    for (int a = 0; a < ORDER; ++a) {
        const long crow = (row0 + ((i - a + ORDER / 2 - 1) & (g.nx - 1))) * g.ny;
        for (int c = 0; c < ORDER; ++c) {
            const long cell = crow + ((j - c + ORDER / 2 - 1) & (g.ny - 1));
            long s0 = start[cell], s1 = start[cell + 1];
            s0 = s0 < 0 ? 0 : s0;
            s1 = s1 > total ? total : s1;
            for (long s = s0; s < s1; ++s) {
                const float* r = rec + (size_t)s * kRec<ORDER>;
                const float w = r[a] * r[ORDER + c];
                const float4 ct = *reinterpret_cast<const float4*>(r + 2 * ORDER);
                const float cv[4] = {ct.x, ct.y, ct.z, ct.w};
#pragma unroll
                for (int f = 0; f < NF; ++f) acc[f] = fma((double)w, (double)cv[f], acc[f]);
            }
        }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) cbar[(size_t)f * nodes + q] = (float)acc[f];
}

// The transpose of ps_particle_spectra_kernel between physical fields: ch [nfields][batch][nx][nh] = rfft2 of the cotangent images (by
// ascending bit of the mask) -> the compact spectra Wb (and Tb with bit 3), [batch][my1][nx].  The map is real, so its transpose takes the
// conjugate multipliers: u^ = i ky w^ / |k|^2 gives -i ky c_u^ / |k|^2, v^ = -i kx w^ / |k|^2 gives i kx c_v^ / |k|^2; the forward's inverse
// transform carries 1 / (nx ny) and the unnormalised forward transform here takes its place, so no factor is left.  Zero outside
// 3 |mx| < nx, as the state's own compaction; (0, 0) of Wb zero (init_vorticity zeroes it), of Tb kept.
__global__ void ps_particle_spectra_adjoint_kernel(const float2* __restrict__ ch, float2* __restrict__ Wb, float2* __restrict__ Tb, int mask,
                                                   int order, int batch, int nx, int ny, int my1, float kx1, float ky1) {
    const long total = (long)batch * my1 * nx, nh = ny / 2 + 1, per = (long)batch * nx * nh;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int i = (int)(q % nx), j = (int)((q / nx) % my1);
        const long b = q / ((long)nx * my1);
        const int mx = i < nx / 2 ? i : i - nx;
        cf w = {0.f, 0.f}, th = w;
        if (3 * (mx < 0 ? -mx : mx) < nx) {
            const size_t at = ((size_t)b * nx + i) * nh + j;
            cf c[4] = {w, w, w, w};
            int slot = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (mask & (1 << k)) { const float2 v = ch[slot * per + at]; c[k] = {v.x, v.y}; ++slot; }
            const float r = (float)(1.0 / (ps_beta(order, mx, nx) * ps_beta(order, j, ny)));
            const float kx = kx1 * (float)mx, ky = ky1 * (float)j, k2 = kx * kx + ky * ky;
            if (k2 > 0.f) {
                const cf psi = imul(-ky, c[0]), phi = imul(kx, c[1]);
                w = {((psi.x + phi.x) / k2 + c[2].x) * r, ((psi.y + phi.y) / k2 + c[2].y) * r};
            }
            th = {c[3].x * r, c[3].y * r};
        }
        if (mask & 7) Wb[q] = make_float2(w.x, w.y);
        if (mask & 8) Tb[q] = make_float2(th.x, th.y);
    }
}

template <int ORDER>
void launch_spread_node(int nfields, dim3 grid, hipStream_t s, const float* rec, const int* start, float* cbar, const PsBox& g) {
    switch (nfields) {
        case 1: hipLaunchKernelGGL((ps_particle_spread_node_kernel<ORDER, 1>), grid, dim3(kPT), 0, s, rec, start, cbar, g); break;
        case 2: hipLaunchKernelGGL((ps_particle_spread_node_kernel<ORDER, 2>), grid, dim3(kPT), 0, s, rec, start, cbar, g); break;
        case 3: hipLaunchKernelGGL((ps_particle_spread_node_kernel<ORDER, 3>), grid, dim3(kPT), 0, s, rec, start, cbar, g); break;
        default: hipLaunchKernelGGL((ps_particle_spread_node_kernel<ORDER, 4>), grid, dim3(kPT), 0, s, rec, start, cbar, g); break;
    }
}

size_t spread_work_bytes(int batch, long npart, int order) { return (size_t)batch * npart * (2 * order + 4) * sizeof(float); }

}  // namespace

NNS_API int nns_spec_ns_particle_cells_i32(const double* pos, int* key, int batch, long npart, int nx, int ny, double Lx, double Ly,
                                           void* stream) {
    const char* who = "spec_ns_particle_cells";
    if (!pos || !key || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (int rc = check_particles(who, batch, npart)) return rc;
    if (int rc = check_particle_box(who, nx, ny, Lx, Ly)) return rc;
    if ((long)batch * nx * ny >= (1L << 31))
        return fail(NNS_ERR_UNSUPPORTED, "%s: batch nx ny = %ld cells must be < 2^31 (the keys are int32)", who, (long)batch * nx * ny);
    const PsBox g{batch, (int)npart, nx, ny, Lx / nx, Ly / ny};
    const dim3 grid((unsigned)(((long)batch * npart + kPT - 1) / kPT));
    hipLaunchKernelGGL(ps_particle_cells_kernel, grid, dim3(kPT), 0, as_stream(stream), pos, key, g);
    return check_launch(who);
}

NNS_API int nns_spec_ns_particle_spread_workspace(int batch, long npart, int order, size_t* bytes) {
    const char* who = "spec_ns_particle_spread_workspace";
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: bytes must be non-NULL and batch >= 1 (batch = %d)", who, batch);
    if (int rc = check_particles(who, batch, npart)) return rc;
    if (int rc = check_order(who, order)) return rc;
    *bytes = spread_work_bytes(batch, npart, order);
    return NNS_OK;
}

NNS_API int nns_spec_ns_particle_spread_f32(const float* cot, const double* pos, const long long* perm, const int* start, float* cbar,
                                            int nfields, int order, void* work, size_t work_bytes_, int batch, long npart, int nx, int ny,
                                            double Lx, double Ly, void* stream) {
    const char* who = "spec_ns_particle_spread";
    if (!cot || !pos || !perm || !start || !cbar || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (int rc = check_particles(who, batch, npart)) return rc;
    if (int rc = check_order(who, order)) return rc;
    if (nfields < 1 || nfields > 4) return fail(NNS_ERR_INVALID_ARG, "%s: nfields = %d must be in [1, 4]", who, nfields);
    if (int rc = check_particle_box(who, nx, ny, Lx, Ly)) return rc;
    if ((long)batch * nx * ny >= (1L << 31))
        return fail(NNS_ERR_UNSUPPORTED, "%s: batch nx ny = %ld cells must be < 2^31", who, (long)batch * nx * ny);
    const size_t need = spread_work_bytes(batch, npart, order);
    if (work_bytes_ < need)
        return fail(NNS_ERR_WORKSPACE, "%s: workspace of %zu bytes, nns_spec_ns_particle_spread_workspace asks for %zu", who, work_bytes_, need);
    const PsBox g{batch, (int)npart, nx, ny, Lx / nx, Ly / ny};
    hipStream_t s = as_stream(stream);
    float* rec = static_cast<float*>(work);
    const dim3 slots((unsigned)(((long)batch * npart + kPT - 1) / kPT)), nodes((unsigned)(((long)batch * nx * ny + kPT - 1) / kPT));
    if (order == 4) hipLaunchKernelGGL(ps_particle_spread_stage_kernel<4>, slots, dim3(kPT), 0, s, cot, pos, perm, rec, nfields, g);
    else hipLaunchKernelGGL(ps_particle_spread_stage_kernel<6>, slots, dim3(kPT), 0, s, cot, pos, perm, rec, nfields, g);
    if (int rc = check_launch(who)) return rc;
    if (order == 4) launch_spread_node<4>(nfields, nodes, s, rec, start, cbar, g);
    else launch_spread_node<6>(nfields, nodes, s, rec, start, cbar, g);
    return check_launch(who);
}

NNS_API int nns_spec_ns_particle_sample_grad_f32(const float* coef, const double* pos, float* grad, int nfields, int order, int batch,
                                                 long npart, int nx, int ny, double Lx, double Ly, void* stream) {
    const char* who = "spec_ns_particle_sample_grad";
    if (!coef || !pos || !grad || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (int rc = check_particles(who, batch, npart)) return rc;
    if (int rc = check_order(who, order)) return rc;
    if (nfields < 1 || nfields > 4) return fail(NNS_ERR_INVALID_ARG, "%s: nfields = %d must be in [1, 4]", who, nfields);
    if (int rc = check_particle_box(who, nx, ny, Lx, Ly)) return rc;
    const PsBox g{batch, (int)npart, nx, ny, Lx / nx, Ly / ny};
    const dim3 grid((unsigned)(((long)batch * npart + kPT - 1) / kPT));
    if (order == 4) hipLaunchKernelGGL(ps_particle_sample_grad_kernel<4>, grid, dim3(kPT), 0, as_stream(stream), coef, pos, grad, nfields, g);
    else hipLaunchKernelGGL(ps_particle_sample_grad_kernel<6>, grid, dim3(kPT), 0, as_stream(stream), coef, pos, grad, nfields, g);
    return check_launch(who);
}

NNS_API int nns_spec_ns_particle_coefs_adjoint_f32(const float* cbar, float* wbar_hat, float* thbar_hat, int fields, int order, void* work,
                                                   size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, void* stream) {
    const char* who = "spec_ns_particle_coefs_adjoint";
    if (!cbar || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (int rc = check_order(who, order)) return rc;
    if (fields < 1 || fields > 15) return fail(NNS_ERR_INVALID_ARG, "%s: fields = %d must be a non-empty mask of bits 0 u, 1 v, 2 w, 3 theta", who, fields);
    if ((fields & 7) && !wbar_hat) return fail(NNS_ERR_INVALID_ARG, "%s: the field mask names u, v or w and wbar_hat is NULL", who);
    if ((fields & 8) && !thbar_hat) return fail(NNS_ERR_INVALID_ARG, "%s: the field mask asks for theta (bit 3) and thbar_hat is NULL", who);
    if (int rc = check_particle_box(who, nx, ny, Lx, Ly)) return rc;
    const int nfields = popcount4(fields);
    const size_t need = particle_work_bytes(batch, nfields, nx, ny);
    if (work_bytes_ < need)
        return fail(NNS_ERR_WORKSPACE, "%s: workspace of %zu bytes, nns_spec_ns_particle_workspace asks for %zu", who, work_bytes_, need);
    if (int rc = nns_spec_rfft2_f32(cbar, static_cast<float*>(work), nfields * batch, nx, ny, stream)) return rc;
    const int my1 = kept_y(ny);
    hipLaunchKernelGGL(ps_particle_spectra_adjoint_kernel, dim3(pw_grid((long)batch * my1 * nx)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2*>(work), reinterpret_cast<float2*>(wbar_hat), reinterpret_cast<float2*>(thbar_hat), fields,
                       order, batch, nx, ny, my1, (float)(2.0 * M_PI / Lx), (float)(2.0 * M_PI / Ly));
    return check_launch(who);
}
