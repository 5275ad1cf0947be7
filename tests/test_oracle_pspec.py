"""CPU checks of the pseudo-spectral solver's restatement (tests/pspec_oracle.py) that the GPU solver (csrc/pspec_kernels.hip,
nns.periodic.PeriodicSolver) is compared against, and of PeriodicSolver's argument checks (raised before any device use)."""
import math

import numpy as np
import pytest

import pspec_cases as C
import pspec_oracle as O
from conftest import rel_l2


def run(S, u0, v0, nsteps):
    w, mean = S.init(u0, v0)
    return S.fields(S.step(w, mean, nsteps), mean)


@pytest.mark.parametrize('nx,ny,Ly', [(64, 64, 2 * np.pi), (64, 256, 4 * np.pi)])
@pytest.mark.parametrize('dt', [0.01, 0.1, 0.5])
def test_taylor_green_is_reproduced_at_any_dt(nx, ny, Ly, dt):
    # J(psi, w) = 0 for Taylor-Green: the nonlinear term vanishes and the integrating factor is exact viscous decay
    nu, rho, n = 0.05, 1.3, 10
    S = O.Scheme(nx, ny, dt, rho, nu, Ly=Ly)
    u0, v0, _ = O.taylor_green(nx, ny, 0.0, nu, rho, Ly=Ly)
    got = run(S, u0, v0, n)
    ref = O.taylor_green(nx, ny, n * dt, nu, rho, Ly=Ly)
    for g, r in zip(got, ref):
        assert np.abs(g - r).max() <= 1e-12


def test_mean_flow_advects_taylor_green():
    U0, V0, nu, dt, n = 0.5, -0.3, 0.01, 0.02, 50
    S = O.Scheme(64, 64, dt, 1.0, nu)
    u0, v0, _ = O.taylor_green(64, 64, 0.0, nu, U0=U0, V0=V0)
    got = run(S, u0, v0, n)
    ref = O.taylor_green(64, 64, n * dt, nu, U0=U0, V0=V0)
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    # RK4 phase error of the advection, (k U dt)^5 / 120 per step at |k U| <= 0.6: ~1e-12 over the run
    assert max(errs) <= 1e-9, errs
    # the same run without the mean is pure decay: the difference is the nonlinear (advection) path
    plain = run(S, *O.taylor_green(64, 64, 0.0, nu)[:2], n)
    assert rel_l2(plain[0] + U0, got[0]) > 1e-2


def test_fourth_order_in_time():
    # 64^2, |m| <= 4, max|u| = 2, nu = 0.01, t = 0.5 in 10 / 20 / 40 steps against 640 steps: measured ratios 16.0 and 16.0
    u0, v0 = O.random_ic(1, 64, 64, 4, seed=1, umax=2.0)
    ref = run(O.Scheme(64, 64, 0.5 / 640, 1.0, 0.01), u0, v0, 640)
    errs = []
    for n in (10, 20, 40):
        got = run(O.Scheme(64, 64, 0.5 / n, 1.0, 0.01), u0, v0, n)
        errs.append(max(rel_l2(g, r) for g, r in zip(got[:2], ref[:2])))
    for a, b in zip(errs, errs[1:]):
        assert 12 <= a / b <= 20, errs


def test_inviscid_energy_and_enstrophy_are_conserved():
    # nu = 0, dt = 0.01, 200 steps at max|u| = 1: measured relative drift 8e-11 (energy) and 3.5e-10 (enstrophy): RK4's O(dt^5) per step
    S = O.Scheme(64, 64, 0.01, 1.0, 0.0)
    u0, v0 = O.random_ic(1, 64, 64, 4, seed=2)
    w, mean = S.init(u0, v0)
    e0, z0 = S.energy(w, mean), S.enstrophy(w)
    w = S.step(w, mean, 200)
    assert abs(S.energy(w, mean) - e0).max() / e0.max() <= 1e-8
    assert abs(S.enstrophy(w) - z0).max() / z0.max() <= 1e-8


def test_output_is_divergence_free_and_init_projects():
    S = O.Scheme(128, 64, 0.01, 1.0, 0.01, Lx=3.0, Ly=1.5)
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal((2, 2, 128, 64))                  # neither divergence-free nor band-limited
    w, mean = S.init(u, v)
    uo, vo, _ = S.fields(w, mean)
    assert np.abs(S.divergence(uo, vo)).max() <= 1e-12 * np.abs(uo).max() * 128
    assert np.allclose(mean, np.stack([u.mean(axis=(1, 2)), v.mean(axis=(1, 2))], axis=-1))
    w2, mean2 = S.init(uo, vo)                                     # a projection: idempotent
    assert np.abs(w2 - w).max() <= 1e-12 * np.abs(w).max()
    uo, vo, _ = S.fields(S.step(w, mean, 5), mean)
    assert np.abs(S.divergence(uo, vo)).max() <= 1e-12 * np.abs(uo).max() * 128


def test_pressure_matches_taylor_green_sign_convention():
    S = O.Scheme(64, 64, 0.1, 2.0, 0.0)
    u, v, p = O.taylor_green(64, 64, 0.0, 0.0, rho=2.0)
    assert np.abs(S.fields(*S.init(u, v))[2] - p).max() <= 1e-13


def _solver(**kw):
    from nns.periodic import PeriodicSolver
    args = dict(nx=64, ny=64, dt=0.01, rho=1.0, nu=0.01)
    args.update(kw)
    return PeriodicSolver(**args)


@pytest.mark.parametrize('kw,exc', [
    (dict(nx=96), ValueError), (dict(ny=2048), ValueError), (dict(nx=32), ValueError), (dict(nx=64.0), TypeError),
    (dict(ny=True), TypeError), (dict(dt=0.0), ValueError), (dict(dt=-1e-3), ValueError), (dict(dt=math.inf), ValueError),
    (dict(rho=0.0), ValueError), (dict(nu=-0.1), ValueError), (dict(nu='0.1'), TypeError), (dict(Lx=0.0), ValueError),
    (dict(Ly=math.nan), ValueError)])
def test_solver_rejects_bad_construction(kw, exc):
    with pytest.raises(exc):
        _solver(**kw)


def test_solver_rejects_bad_calls_before_any_device_use():
    s = _solver(nx=64, ny=128, Ly=4 * np.pi)
    assert s.my1 == 43 and s.last_simulate_used_graph is False
    f64 = np.zeros((2, 64, 128))
    f32 = np.zeros((2, 64, 128), dtype=np.float32)
    with pytest.raises(TypeError):
        s.init(f64, f64)
    with pytest.raises(TypeError):
        s.init(f32, [[0.0]])
    with pytest.raises(ValueError):
        s.init(np.zeros((2, 128, 64), dtype=np.float32), np.zeros((2, 128, 64), dtype=np.float32))
    with pytest.raises(TypeError):
        s.step(object())
    with pytest.raises(TypeError):
        s.fields(None)
    with pytest.raises(ValueError):
        s.simulate(f32, f32, nsteps=10, save_every=3)
    with pytest.raises(ValueError):
        s.simulate(f32, f32, nsteps=-1)
    with pytest.raises(ValueError):
        s.simulate(f32, f32, nsteps=4, save_every=0)
    with pytest.raises(TypeError):
        s.simulate(f32, f32, nsteps=4.0)
    e = s.residual_engine(every=5)
    assert (e.nx, e.ny, e.backend) == (64, 128, 'spectral') and abs(e.dt - 0.05) < 1e-15 and e.Ly == 4 * np.pi
    with pytest.raises(ValueError):
        s.residual_engine(every=0)


def test_state_layout_helper():
    S = O.Scheme(64, 128, 0.01, 1.0, 0.0)
    w, _ = S.init(*O.random_ic(3, 64, 128, 8, seed=4))
    c = S.compact(w)
    assert c.shape == (3, 43, 64) and np.array_equal(c[1, 5, 7], w[1, 7, 5])
    assert np.abs(w[..., 43:]).max() == 0                           # nothing outside the kept columns


# ---------------------------------------------------------------------------------------------------- full-band cases (pspec_cases.py)
@pytest.mark.parametrize('case', C.FULL_BAND, ids=[C.case_id(c) for c in C.FULL_BAND])
def test_band_ic_fills_the_band(case):
    nx, ny, B, Lx, Ly, mean = case
    u, v = O.band_ic(B, nx, ny, C.seed(case), Lx, Ly, C.UMAX, mean)
    assert np.isclose(max(np.abs(u - mean[0]).max(), np.abs(v - mean[1]).max()), C.UMAX)
    assert np.allclose(u.mean(axis=(1, 2)), mean[0]) and np.allclose(v.mean(axis=(1, 2)), mean[1])
    S = O.Scheme(nx, ny, 0.01, 1.0, 0.0, Lx, Ly)
    kmax = max(np.pi * nx / Lx, np.pi * ny / Ly)
    assert np.abs(S.divergence(u, v)).max() <= 1e-12 * kmax
    # Hermitian-consistent: every drawn coefficient survives irfft2 (the m_y = 0 column is conjugate-symmetric in m_x)
    psi = O.band_psi(B, nx, ny, C.seed(case))
    uh = np.fft.rfft2(u - mean[0])
    want = 1j * S.ky * psi
    scale = np.vdot(want, uh).real / np.vdot(want, want).real
    assert np.linalg.norm(uh - scale * want) <= 1e-12 * np.linalg.norm(uh)
    # band-limited, and the outermost kept shell of each axis (|m_x| = (nx - 1) // 3, m_y = my1 - 1) carries energy: measured over
    # these shapes 4.0e-4 .. 6.4e-3 of the total in each (random_ic with |m| <= 8 has none there)
    e = np.abs(uh) ** 2 + np.abs(np.fft.rfft2(v - mean[1])) ** 2
    inside = O.band(nx, ny)
    assert e[:, ~inside].sum() <= 1e-28 * e.sum()
    mx = np.abs(np.fft.fftfreq(nx) * nx)
    ex = e[:, mx == (nx - 1) // 3].sum() / e.sum()
    ey = e[:, :, O.kept_y(ny) - 1].sum() / e.sum()
    assert ex >= 2.5e-4 and ey >= 2.5e-4, (ex, ey)


def _mutation_errors(u0, v0, dt, nx, ny, Lx, Ly, nsteps, nu):
    _, ref = C.oracle_run(u0, v0, dt, nx, ny, Lx, Ly, nsteps, nu)
    out = {}
    for name, widen in (('x', (1, 0)), ('y', (0, 1))):
        _, got = C.oracle_run(u0, v0, dt, nx, ny, Lx, Ly, nsteps, nu, widen)
        out[name] = [rel_l2(g, r) for g, r in zip(got, ref)]
    return out


# the GPU cases of pspec_cases.FULL_BAND at B = 1 and axes cut to <= 256 (CPU cost), each box, mean and dt rule kept
REDUCED = sorted(set((min(c[0], 256), min(c[1], 256), 1, c[3], c[4], c[5]) for c in C.FULL_BAND))


@pytest.mark.parametrize('case', REDUCED, ids=[C.case_id(c) + '_L%.3g' % c[3] for c in REDUCED])
def test_full_band_cases_detect_a_mask_one_mode_too_wide(case):
    # a dealiasing mask that keeps one more mode, in x (3 (|m_x| - 1) < nx) or in y (j < my1 + 1), moves the velocity of these cases by
    # >= 100x the GPU bound BOUND_UV (2e-6; the GPU measured <= 6.4e-7).  Measured here, the larger of u and v: 7.0e-3 .. 3.2e-2 (x),
    # 2.7e-3 .. 2.8e-2 (y).
    # (The stiff case of the GPU tests cannot tell: no energy reaches the band edge there, so the extra mode stays empty.)
    nx, ny, B, Lx, Ly, mean = case
    u0, v0, dt = C.full_band_input(*case)
    errs = _mutation_errors(u0, v0, dt, nx, ny, Lx, Ly, C.NSTEPS, C.NU)
    print('%dx%d mask one mode too wide: rel-L2 u, v, p  x %s  y %s' % (nx, ny, ['%.1e' % e for e in errs['x']], ['%.1e' % e for e in errs['y']]))
    for name in errs:
        assert max(errs[name][:2]) >= 100 * C.BOUND_UV, (name, errs)


def test_band_limited_case_cannot_detect_a_mask_one_mode_too_wide():
    # the case of tests/test_gpu_pspec.py::test_random_band_limited_ic_against_the_oracle (|m| <= 8: products inside |m| <= 16, far
    # inside the band) moves by 4.2e-6 (x) and 2.6e-6 (y) under the same mask errors: inside its 5e-6 bound, hence the full-band cases
    u0, v0 = O.random_ic(4, 128, 128, 8, seed=11, umax=2.0)
    u0, v0 = u0.astype(np.float32), v0.astype(np.float32)
    errs = _mutation_errors(u0, v0, 0.005, 128, 128, 2 * np.pi, 2 * np.pi, 50, 0.01)
    print('|m| <= 8 case, mask one mode too wide: x %s  y %s' % (['%.1e' % e for e in errs['x']], ['%.1e' % e for e in errs['y']]))
    assert max(errs['x']) <= 5e-6 and max(errs['y']) <= 5e-6, errs
    assert max(errs['x']) >= 1e-6 and max(errs['y']) >= 1e-6, errs             # the variants do run a different scheme


def test_inviscid_case_detects_a_mask_one_mode_too_wide():
    # the inviscid GPU case (tests/test_gpu_pspec_edges.py: 128^2 full band, 200 steps, energy and enstrophy drift <= 5e-6; the GPU
    # measured 5.7e-7): a mask one mode too wide breaks the conservation of the dealiased scheme.  Measured: the larger drift is
    # 1.5e-4 (x) and 3.4e-4 (y)
    n = 128
    u0, v0 = O.band_ic(1, n, n, seed=5)
    u0, v0 = u0.astype(np.float32), v0.astype(np.float32)
    dt = O.cfl_dt(n, n, 2 * np.pi, 2 * np.pi, 1.0)
    for widen in ((0, 0), (1, 0), (0, 1)):
        S = O.Scheme(n, n, dt, 1.0, 0.0, widen=widen)
        w, mean = S.init(u0, v0)
        e0, z0 = S.energy(w, mean), S.enstrophy(w)
        w = S.step(w, mean, 200)
        drift = max((abs(S.energy(w, mean) - e0) / e0).max(), (abs(S.enstrophy(w) - z0) / z0).max())
        print('inviscid 128^2, widen', widen, 'drift %.2e' % drift)
        assert drift <= 1e-6 if widen == (0, 0) else drift >= 20 * 5e-6, (widen, drift)
