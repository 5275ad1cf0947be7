// The kernels of K tangents on the scalar and the buoyant step (nns_spec_ns_step_scalar_tangents_f32) as a translation unit of their own, on
// the pattern of pspec_scalar_tangent.hip: the text of pspec_kernels.hip, which under this macro leaves its host entry points out, names only
// the forms with a PsTangentsScalar in launch_col_stage and defines ps_scalar_tangents_col / ps_scalar_tangents_row for the driver in
// pspec_kernels.o to call.  The scalar half of the pairs' inner product lives here too, kernel and entry point, so that pspec_kernels.o is
// what it was.
#define PSPEC_SCALAR_TANGENTS_TU
#include "pspec_kernels.hip"

namespace {

// out[b][k][l] (float64) = 1/2 sum wt Re(conj(dtheta_k) dtheta_l) / (nx ny)^2 over the stored modes of grid b but (0, 0): the variance inner
// product of members k and l of D [K][B][my1][nx], ps_tangent_gram_kernel's twin (its walk, float64 sums, shuffle tree and index-ordered
// partials; one workgroup per (grid, pair k <= l), both triangles written, no atomics).  The term is spelt as ps_scalar_diag_kernel spells its
// variance, so the diagonal is bitwise column 0 of nns_spec_ns_scalar_diag_f32 of each member.  The (0, 0) entry, the mean of dtheta, is not read.
__global__ __launch_bounds__(kDiagT) void ps_tangent_variance_gram_kernel(const float2* __restrict__ D, double* __restrict__ out, int K, long kstride,
                                                                          int nx, int my1, double inv_n2) {
    __shared__ double part[kDiagT / kWave];
    int k = 0, rem = (int)blockIdx.x;                       // pair index -> (k, l), k <= l: row k holds K - k pairs
    while (rem >= K - k) { rem -= K - k; ++k; }
    const int l = k + rem;
    const long per = (long)my1 * nx;
    const float2* dk = D + (size_t)k * kstride + (size_t)blockIdx.y * per;
    const float2* dl = D + (size_t)l * kstride + (size_t)blockIdx.y * per;
    double e = 0.;
    for (long q = threadIdx.x; q < per; q += kDiagT) {
        const int j = (int)(q / nx);
        const double wt = j == 0 ? 1. : 2.;
        const float2 c = q > 0 ? dk[q] : make_float2(0.f, 0.f), d = q > 0 ? dl[q] : make_float2(0.f, 0.f);      // q = 0 is the (0, 0) mode: |k|^2 > 0 elsewhere
        const double tt = q > 0 ? (double)c.x * d.x + (double)c.y * d.y : 0.;
        e += wt * tt;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) e += __shfl_xor(e, d, kWave);
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) part[wave] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double se = 0.;
        for (int w = 0; w < kDiagT / kWave; ++w) se += part[w];
        double* o = out + (size_t)blockIdx.y * K * K;
        o[(size_t)k * K + l] = o[(size_t)l * K + k] = 0.5 * se * inv_n2;
    }
}

}  // namespace

NNS_API int nns_spec_ns_tangent_variance_gram_f64(const float* dthat, int ntan, double* out, int batch, int nx, int ny, void* stream) {
    const char* who = "spec_ns_tangent_variance_gram";
    if (!dthat || !out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (ntan < 1 || ntan > kMaxTangents) return fail(NNS_ERR_INVALID_ARG, "%s: ntan = %d must be in [1, %d]", who, ntan, kMaxTangents);
    if (int rc = check_axes(who, nx, ny)) return rc;
    const int my1 = kept_y(ny);
    const double n = (double)nx * ny;
    hipLaunchKernelGGL(ps_tangent_variance_gram_kernel, dim3(ntan * (ntan + 1) / 2, batch), dim3(kDiagT), 0, as_stream(stream),
                       reinterpret_cast<const float2*>(dthat), out, ntan, (long)batch * my1 * nx, nx, my1, 1.0 / (n * n));
    return check_launch("spec_ns_tangent_variance_gram");
}
