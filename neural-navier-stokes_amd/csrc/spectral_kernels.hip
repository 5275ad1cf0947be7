// Fourier-spectral back-end of the periodic Navier-Stokes residual, gfx950: the whole-grid entry points (kernels: spectral_fwd.h).
// Operator definition: oracle/periodic.py (spectral_residual); no reference symbol exists.
#include "spectral_fwd.h"

using namespace nns;
using namespace nns::spec;

namespace {

int xpass(const float* u, const float* v, const float* p, float* ru, float* rv, float* rd, int batch, int nx, int ny,
          double Lx, double rho, double nu, int precise, hipStream_t s) {
    if (!u || !v || !p || !ru || !rv || !rd || batch < 1 || ny < 1) return fail(NNS_ERR_INVALID_ARG, "spec_residual_xpass: bad args");
    if (Lx == 0 || rho == 0) return fail(NNS_ERR_INVALID_ARG, "spec_residual_xpass: Lx, rho must be non-zero");
    if (!pow2_in_range(nx)) return dense_xpass(u, v, p, ru, rv, rd, batch, nx, ny, Lx, rho, nu, s);          // any other length 3 .. 2048: circulant matrices, float64
    return xpass_fft<false>(u, v, p, ru, rv, rd, batch, nx, ny, Lx, rho, nu, precise, s);
}

int ypass(const float* u, const float* v, const float* p, const float* up, const float* vp, float* ru, float* rv, float* rd,
          int batch, int nx, int ny, double dt, double Ly, double rho, double nu, int precise, hipStream_t s) {
    if (!u || !v || !p || !up || !vp || !ru || !rv || !rd || batch < 1 || nx < 1) return fail(NNS_ERR_INVALID_ARG, "spec_residual_ypass: bad args");
    if (Ly == 0 || rho == 0 || dt == 0) return fail(NNS_ERR_INVALID_ARG, "spec_residual_ypass: Ly, rho, dt must be non-zero");
    if (!pow2_in_range(ny)) return dense_ypass(u, v, p, up, vp, ru, rv, rd, batch, nx, ny, dt, Ly, rho, nu, s);
    return ypass_fft<false>(u, v, p, up, vp, ru, rv, rd, batch, nx, ny, dt, Ly, rho, nu, precise, s);
}

// FD 5-point + spectral residual of the same inputs: spectral x-pass, then the row pass with the stencil fused in.
int residual_both(const float* u, const float* v, const float* p, const float* up, const float* vp, float* fu, float* fv, float* fd,
                  float* ru, float* rv, float* rd, int batch, int nx, int ny, double dt, double Lx, double Ly, double rho, double nu,
                  int precise, hipStream_t s, bool with_xpass, const float* halo_top = nullptr, const float* halo_bot = nullptr, long halo_fstride = 0) {
    if (!u || !v || !p || !up || !vp || !fu || !fv || !fd || !ru || !rv || !rd || batch < 1 || nx < 3)
        return fail(NNS_ERR_INVALID_ARG, "residual_both: bad args");
    const bool slab = halo_top || halo_bot;               // a row slab: nx is the LOCAL row count (any value >= 3), only ny is transformed here
    if (slab && (!halo_top || !halo_bot || with_xpass)) return fail(NNS_ERR_INVALID_ARG, "residual_both: a row slab needs both halo messages and the row pass only");
    if (Ly == 0 || rho == 0 || dt == 0 || Lx == 0) return fail(NNS_ERR_INVALID_ARG, "residual_both: Lx, Ly, rho, dt must be non-zero");
    if (with_xpass) precise = spec_resolve_precise(precise, nu, nx, Lx, ny, Ly);       // a whole evaluation: one arithmetic for both passes
    if (!slab && (!spec_len_ok(nx) || !spec_len_ok(ny)))
        return fail(NNS_ERR_UNSUPPORTED, "residual_both: nx=%d, ny=%d: powers of two in [64, 1024] (FFT engine) or any length 3 .. %d (dense fallback)", nx, ny, kDenseMaxLen);
    if (!pow2_in_range(ny) && !slab) {
        // rows the FFT engine does not serve: no fused row pass -- the standalone stencil kernel, then the spectral passes (dense where needed)
        if (int rc = nns_fd_residual_f32(u, v, p, up, vp, fu, fv, fd, batch, nx, ny, dt, Lx / nx, Ly / ny, rho, nu, 5, s)) return rc;
        if (with_xpass) { if (int rc = xpass(u, v, p, ru, rv, rd, batch, nx, ny, Lx, rho, nu, precise, s)) return rc; }
        return ypass(u, v, p, up, vp, ru, rv, rd, batch, nx, ny, dt, Ly, rho, nu, precise, s);
    }
    if (!pow2_in_range(ny)) return fail(NNS_ERR_UNSUPPORTED, "residual_both (row slab): ny=%d must be a power of two in [64, 1024]", ny);
    if (with_xpass) {
        // (the two launches per group of G grids, so that a group's row pass finds its partials in the Infinity Cache, were tried: slower at every G,
        // profiles/r04_grouped_launches.txt)
        if (int rc = xpass(u, v, p, ru, rv, rd, batch, nx, ny, Lx, rho, nu, precise, s)) return rc;
    }
    const double dx = slab ? Lx : Lx / nx;                                              // a row slab passes the grid spacing itself in Lx
    return fused_rowpass<false>(u, v, p, up, vp, fu, fv, fd, ru, rv, rd, batch, nx, ny, dt, dx, Ly, rho, nu, precise,
                                make_halo_k(halo_top, halo_bot, halo_fstride, batch, ny), s);
}

}  // namespace

NNS_API int nns_residual_both_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                  float* fd_r_u, float* fd_r_v, float* fd_r_div, float* sp_r_u, float* sp_r_v, float* sp_r_div,
                                  int batch, int nx, int ny, double dt, double Lx, double Ly, double rho, double nu, int precise, void* stream) {
    return residual_both(u, v, p, u_prev, v_prev, fd_r_u, fd_r_v, fd_r_div, sp_r_u, sp_r_v, sp_r_div, batch, nx, ny, dt, Lx, Ly, rho, nu, precise, as_stream(stream), true);
}
NNS_API int nns_residual_both_rowpass_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                          float* fd_r_u, float* fd_r_v, float* fd_r_div, float* sp_r_u, float* sp_r_v, float* sp_r_div,
                                          int batch, int nx, int ny, double dt, double Lx, double Ly, double rho, double nu, int precise, void* stream) {
    return residual_both(u, v, p, u_prev, v_prev, fd_r_u, fd_r_v, fd_r_div, sp_r_u, sp_r_v, sp_r_div, batch, nx, ny, dt, Lx, Ly, rho, nu, precise, as_stream(stream), false);
}

NNS_API int nns_residual_both_rowpass_halo_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                               const float* halo_top, const float* halo_bot,
                                               float* fd_r_u, float* fd_r_v, float* fd_r_div, float* sp_r_u, float* sp_r_v, float* sp_r_div,
                                               int batch, int nx_local, int ny, long halo_field_stride, double dt, double dx, double Ly, double rho, double nu,
                                               int precise, void* stream) {
    if (int rc = check_halo("residual_both_rowpass_halo", halo_top, halo_bot, halo_field_stride, batch, ny)) return rc;
    return residual_both(u, v, p, u_prev, v_prev, fd_r_u, fd_r_v, fd_r_div, sp_r_u, sp_r_v, sp_r_div, batch, nx_local, ny, dt, dx, Ly, rho, nu, precise,
                         as_stream(stream), false, halo_top, halo_bot, halo_field_stride);
}
NNS_API int nns_spec_residual_xpass_f32(const float* u, const float* v, const float* p, float* r_u, float* r_v, float* r_div,
                                        int batch, int nx, int ny, double Lx, double rho, double nu, int precise, void* stream) {
    return xpass(u, v, p, r_u, r_v, r_div, batch, nx, ny, Lx, rho, nu, precise, as_stream(stream));
}
NNS_API int nns_spec_residual_ypass_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                        float* r_u, float* r_v, float* r_div, int batch, int nx, int ny, double dt, double Ly,
                                        double rho, double nu, int precise, void* stream) {
    return ypass(u, v, p, u_prev, v_prev, r_u, r_v, r_div, batch, nx, ny, dt, Ly, rho, nu, precise, as_stream(stream));
}
NNS_API int nns_spec_residual_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                  float* r_u, float* r_v, float* r_div, int batch, int nx, int ny, double dt, double Lx, double Ly,
                                  double rho, double nu, int precise, void* stream) {
    if (!spec_len_ok(nx) || !spec_len_ok(ny))                  // before the first launch: both axes must have an engine
        return fail(NNS_ERR_UNSUPPORTED, "spec_residual: nx=%d, ny=%d: powers of two in [64, 1024] (FFT engine) or any length 3 .. %d (dense fallback)", nx, ny, kDenseMaxLen);
    const int pr = spec_resolve_precise(precise, nu, nx, Lx, ny, Ly);       // one arithmetic for both passes
    if (int rc = xpass(u, v, p, r_u, r_v, r_div, batch, nx, ny, Lx, rho, nu, pr, as_stream(stream))) return rc;
    return ypass(u, v, p, u_prev, v_prev, r_u, r_v, r_div, batch, nx, ny, dt, Ly, rho, nu, pr, as_stream(stream));
}

// The arithmetic a `precise` request resolves to for a whole evaluation (0 = all-float32 transforms, 2 = float64 forward transforms): hosts that
// call the passes one by one -- the slab-decomposed path, nns/slab.py -- ask once and hand the answer to every pass, so that there is ONE policy
// implementation (NNS_SPEC_F64 included).
NNS_API int nns_spec_resolve_precise(int precise, double nu, int nx, double Lx, int ny, double Ly) {
    return spec_resolve_precise(precise, nu, nx, Lx, ny, Ly);
}
