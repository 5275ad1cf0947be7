"""GPU checks of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip through nns.periodic.PeriodicSolver) where its kernels can
go wrong and tests/test_gpu_pspec.py does not look: flows whose spectrum fills the whole 2/3 band (the dealiasing masks and the Hermitian
packing at the band edge), every template on each axis, extreme aspect ratios, the grid-stride loops, the inviscid, stiff and
tiny-viscosity regimes and non-default streams.  The reference is the float64 restatement tests/pspec_oracle.py."""
import numpy as np
import pytest
import torch

import pspec_cases as C
import pspec_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(ts):
    return [t.cpu().numpy().astype(np.float64) for t in ts]


def solver(nx, ny, dt, nu, Lx=TWO_PI, Ly=TWO_PI, rho=C.RHO):
    from nns.periodic import PeriodicSolver
    return PeriodicSolver(nx, ny, dt, rho, nu, Lx=Lx, Ly=Ly)


def state_c(st):
    w = st.what.cpu().numpy().astype(np.float64)
    return w[..., 0] + 1j * w[..., 1]


def expand(S, wc):
    """The solver's compact state [..., my1, nx] -> the rfft2 layout [..., nx, nh] (zero past the kept columns)."""
    w = np.zeros(wc.shape[:-2] + (S.nx, S.ny // 2 + 1), dtype=np.complex128)
    w[..., :O.kept_y(S.ny)] = np.swapaxes(wc, -1, -2)
    return w


def dropped_x(nx):
    """Indices i (fftfreq order) of the x-wavenumbers the 2/3 rule drops: 3|m_x| >= nx."""
    mx = np.abs(np.fft.fftfreq(nx) * nx)
    return np.nonzero(3 * mx >= nx)[0]


def check_exact_zeros(st, nx):
    what = st.what.cpu()
    assert torch.count_nonzero(what[:, :, dropped_x(nx), :]) == 0          # the column pass writes literal zeros outside the band
    assert torch.count_nonzero(what[:, 0, 0, :]) == 0                       # and at (0, 0): the mean flow lives in `mean`


# ---------------------------------------------------------------------------------------------------- a. full band, every shape
@pytest.mark.parametrize('case', C.FULL_BAND, ids=[C.case_id(c) for c in C.FULL_BAND])
def test_full_band_step_against_the_oracle(gpu_device, case):
    nx, ny, B, Lx, Ly, mean = case
    u0, v0, dt = C.full_band_input(*case)
    w, ref = C.oracle_run(u0, v0, dt, nx, ny, Lx, Ly)
    s = solver(nx, ny, dt, C.NU, Lx, Ly)
    st = s.init(dev(u0), dev(v0))
    s.step(st, C.NSTEPS)
    got = host(s.fields(st))
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    ew = rel_l2(state_c(st), O.Scheme(nx, ny, dt, C.RHO, C.NU, Lx, Ly).compact(w))
    print('full band %dx%d B=%d dt=%.2e, %d steps: rel-L2 u, v, p %s, what %.2e' % (nx, ny, B, dt, C.NSTEPS, ['%.2e' % e for e in errs], ew))
    # measured on the MI355X (u, v, p, what): 64x64 2.1e-7 2.0e-7 1.2e-6 2.4e-7; 128x512 3.1e-7 3.0e-7 4.9e-6 2.5e-7;
    # 512x128 3.1e-7 2.9e-7 1.0e-5 2.6e-7; 512x512 3.4e-7 3.3e-7 4.6e-6 2.7e-7; 256x1024 3.1e-7 4.0e-7 3.3e-6 2.7e-7;
    # 1024x256 3.1e-7 3.2e-7 3.5e-6 2.8e-7; 1024x64 3.7e-7 3.2e-7 1.2e-6 2.8e-7; 64x1024 3.1e-7 6.4e-7 9.1e-7 2.7e-7.
    # Bounds in pspec_cases.py; a mask one mode too wide moves u or v by >= 100x BOUND_UV on these cases
    # (tests/test_oracle_pspec.py::test_full_band_cases_detect_a_mask_one_mode_too_wide)
    assert max(errs[:2]) <= C.BOUND_UV and errs[2] <= C.BOUND_P and ew <= C.BOUND_W, (errs, ew)
    check_exact_zeros(st, nx)
    assert np.abs(st.mean.cpu().numpy() - np.array(mean)).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------- b. physical regimes
def test_inviscid_full_band_against_the_oracle_and_conserves(gpu_device):
    n, steps, check_at = 128, 200, 20
    u0, v0 = O.band_ic(1, n, n, seed=5)
    u0, v0 = u0.astype(np.float32), v0.astype(np.float32)
    dt = O.cfl_dt(n, n, TWO_PI, TWO_PI, 1.0)
    S = O.Scheme(n, n, dt, C.RHO, 0.0)
    w0, mean = S.init(u0, v0)
    s = solver(n, n, dt, 0.0)
    st = s.init(dev(u0), dev(v0))
    e0, z0 = S.energy(expand(S, state_c(st)), mean), S.enstrophy(expand(S, state_c(st)))
    s.step(st, check_at)
    ref = S.fields(S.step(w0, mean, check_at), mean)
    errs = [rel_l2(g, r) for g, r in zip(host(s.fields(st)), ref)]
    s.step(st, steps - check_at)
    wg = expand(S, state_c(st))
    de, dz = (abs(S.energy(wg, mean) - e0) / e0).max(), (abs(S.enstrophy(wg) - z0) / z0).max()
    print('inviscid 128^2 full band: rel-L2 u, v, p after %d steps %s; drift over %d steps: energy %.2e enstrophy %.2e'
          % (check_at, ['%.2e' % e for e in errs], steps, de, dz))
    # measured on the MI355X: u, v, p 2.9e-7, 3.0e-7, 2.2e-6; drift energy 5.7e-7, enstrophy 5.5e-7 (the float64 scheme's own:
    # 9.4e-8 and 5.2e-7, RK4's O(dt^5) per step).  A mask one mode too wide drifts 2e-5 .. 3e-4 and moves u, v by 0.3 (CPU, 200 steps)
    assert max(errs[:2]) <= 2e-6 and errs[2] <= 2e-5, errs
    assert de <= 5e-6 and dz <= 5e-6, (de, dz)
    check_exact_zeros(st, n)


def test_stiff_viscosity_against_the_oracle(gpu_device):
    n, steps = 128, 20
    u0, v0 = O.band_ic(2, n, n, seed=6, mean=(0.1, 0.2))
    u0, v0 = u0.astype(np.float32), v0.astype(np.float32)
    dt = O.cfl_dt(n, n, TWO_PI, TWO_PI, 1.2)
    kmax = (n - 1) // 3                                  # 2 pi / L = 1
    nu = 60.0 / (kmax * kmax * dt)
    assert nu * kmax * kmax * dt >= 50                   # the edge modes decay by exp(-60) and more per step
    _, ref = C.oracle_run(u0, v0, dt, n, n, TWO_PI, TWO_PI, steps, nu)
    s = solver(n, n, dt, nu)
    st = s.init(dev(u0), dev(v0))

    def edge_modes(wc):                                  # the outermost kept shell of each axis: |m_x| = kmax and m_y = my1 - 1
        return max(np.abs(wc[:, :, kmax]).max(), np.abs(wc[:, :, n - kmax]).max(), np.abs(wc[:, -1, :]).max())
    edge0 = edge_modes(state_c(st))
    s.step(st, steps)
    got = host(s.fields(st))
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    edge = edge_modes(state_c(st))
    print('stiff 128^2 nu = %.3g (nu k_max^2 dt = 60): rel-L2 u, v, p %s; edge modes %.2e -> %.2e' % (nu, ['%.2e' % e for e in errs], edge0, edge))
    # measured on the MI355X: u, v, p 3.3e-7, 1.1e-7, 5.3e-7; edge modes 2.7e3 -> 1.6e-9 (float32 rounding of the products; the
    # oracle's end at ~4e-22 of their start).  No energy reaches the band edge here, so this case cannot see a mask error
    assert max(errs[:2]) <= 2e-6 and errs[2] <= 5e-6, errs
    assert edge <= 5e-12 * edge0, (edge0, edge)
    check_exact_zeros(st, n)


def test_tiny_viscosity_taylor_green_decay(gpu_device):
    # nu = 1e-5: the decay per step, nu |k|^2 dt = 1.5e-7 on the Taylor-Green modes, is ~1.5 ulp of the float32 state, so the state's
    # own rounding bounds the agreement with the analytic decay.  The kernel applies it as fmaf(expm1(L dt), w, w), one correctly
    # rounded update per step: the (1, 1) modes must follow that float32 recurrence.  A kernel that multiplied by the rounded
    # E^2 = exp(L dt) instead would follow another recurrence, >= 10x the tolerance away (asserted below).
    n, nu, dt, steps, amp = 128, 1e-5, 0.0075, 1000, 0.9
    u0, v0, _ = O.taylor_green(n, n, 0.0, nu)
    s = solver(n, n, dt, nu)
    st = s.init(dev(amp * u0), dev(amp * v0))
    z0 = st.what[0, 1, [1, n - 1], 0].cpu().numpy()                  # Re w^ at (m_x, m_y) = (+-1, 1)
    s.step(st, steps)
    z = st.what[0, 1, [1, n - 1], 0].cpu().numpy()
    got = host(s.fields(st))
    ref = O.taylor_green(n, n, steps * dt, nu)
    errs = [rel_l2(g, amp * r) for g, r in zip(got[:2], ref[:2])] + [rel_l2(got[2], amp * amp * ref[2])]
    x2 = np.float32(2) * (np.float32(-0.5 * nu * dt) * np.float32(2))         # L dt on |k|^2 = 2, as the kernel forms it
    em2, e2 = np.float32(np.expm1(np.float64(x2))), np.float32(np.exp(np.float64(x2)))
    fma, rounded = z0.astype(np.float32), z0.astype(np.float32)
    for _ in range(steps):
        fma = (fma.astype(np.float64) * (1 + np.float64(em2))).astype(np.float32)
        rounded = rounded * e2
    exact = z0 * np.exp(np.float64(x2) * steps)
    d_fma, d_rounded = np.abs(z - fma).max() / np.abs(z0).max(), np.abs(rounded - fma).max() / np.abs(z0).max()
    print('Taylor-Green nu = 1e-5, %d steps: rel-L2 u, v, p vs analytic %s; (1, 1) modes vs the fma recurrence %.2e, vs exact %.2e; '
          'rounded-E recurrence vs fma %.2e' % (steps, ['%.2e' % e for e in errs], d_fma, np.abs(z - exact).max() / np.abs(z0).max(), d_rounded))
    # measured on the MI355X: the modes equal the fma recurrence exactly (0 difference); the rounded-E recurrence is 6.6e-5 away;
    # u, v, p against the analytic decay 1.75e-5, 1.75e-5, 3.5e-5 -- all of it the float32 state's rounding (the fma recurrence's own
    # distance from exact decay is the same 1.75e-5)
    tol = 1e-6
    assert d_rounded >= 10 * tol, d_rounded
    assert d_fma <= tol, (z, fma, rounded)
    assert max(errs[:2]) <= 5e-5 and errs[2] <= 1e-4, errs


# ---------------------------------------------------------------------------------------------------- c. grid-stride loops
def test_grid_stride_1024_by_32_members_are_the_single_runs(gpu_device):
    # 1024^2 x 32: row pass 32768 lines / 4 per tile = 8192 tiles, column pass 32 * 342 = 10944 lines / 4 = 2736 tiles, both on 2048
    # workgroups; the pointwise kernels (init, derivs, source, pressure) exceed 4096 x 256 threads.  Member 23's columns (lines
    # 7866..8207) straddle line 8192, the first tile a workgroup takes on its second trip; members >= 8 are on the row pass's second trip
    n, B, steps = 1024, 32, 3
    dt = O.cfl_dt(n, n, TWO_PI, TWO_PI, 1.0)
    ics = [O.band_ic(1, n, n, seed=100 + k) for k in range(B)]
    u0 = np.concatenate([a[0] for a in ics]).astype(np.float32)
    v0 = np.concatenate([a[1] for a in ics]).astype(np.float32)
    del ics
    s = solver(n, n, dt, C.NU)
    st = s.init(dev(u0), dev(v0))
    s.step(st, steps)
    outs = s.fields(st)
    try:
        for k in (0, 1, 23, 31):
            one = s.init(dev(u0[k:k + 1]), dev(v0[k:k + 1]))
            s.step(one, steps)
            assert torch.equal(one.what[0], st.what[k]), k
            for a, b in zip(s.fields(one), outs):
                assert torch.equal(a[0], b[k]), k
            del one
        check_exact_zeros(st, n)
        for k in (0, 31):
            _, ref = C.oracle_run(u0[k], v0[k], dt, n, n, TWO_PI, TWO_PI, steps)
            errs = [rel_l2(o[k].cpu().numpy(), r) for o, r in zip(outs, ref)]
            print('1024^2 x 32, member %d, %d steps: rel-L2 u, v, p %s' % (k, steps, ['%.2e' % e for e in errs]))
            assert max(errs[:2]) <= C.BOUND_UV and errs[2] <= C.BOUND_P, (k, errs)
    finally:
        del st, outs
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- d. streams
def test_non_default_stream_is_bitwise_the_default_stream(gpu_device):
    nx, ny, steps = 128, 256, 5
    u0, v0 = O.band_ic(2, nx, ny, seed=8, Ly=2 * TWO_PI)
    u0, v0 = u0.astype(np.float32), v0.astype(np.float32)
    dt = O.cfl_dt(nx, ny, TWO_PI, 2 * TWO_PI, 1.0)
    s = solver(nx, ny, dt, C.NU, Ly=2 * TWO_PI)
    st = s.init(dev(u0), dev(v0))
    s.step(st, steps)
    ref = s.fields(st)
    src_u, src_v = dev(u0), dev(v0)
    u, v = torch.zeros_like(src_u), torch.zeros_like(src_v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the side stream holds its inputs back: work that ran on any other stream would read zeros
        torch.cuda._sleep(20_000_000)
        u.copy_(src_u)
        v.copy_(src_v)
        st2 = s.init(u, v)
        s.step(st2, steps)
        got = s.fields(st2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(st2.what, st.what) and torch.equal(st2.mean, st.mean)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
