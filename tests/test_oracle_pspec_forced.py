"""CPU checks of the forced restatement (tests/pspec_forced_oracle.py) that the GPU solver's forced step and diagnostics
(csrc/pspec_kernels.hip: nns_spec_ns_step_forced_f32, nns_spec_ns_diag_f32) are compared against, and of PeriodicSolver's argument
checks for drag and forcing (raised before any device use)."""
import math

import numpy as np
import pytest

import pspec_cases as C
import pspec_forced_cases as FC
import pspec_forced_oracle as F
import pspec_oracle as O
from conftest import rel_l2

TWO_PI = 2 * np.pi


def run(S, u0, v0, nsteps):
    w, mean = S.init(u0, v0)
    return S.fields(S.step(w, mean, nsteps), mean)


def test_without_force_and_drag_it_is_the_parent_exactly():
    u0, v0 = O.random_ic(2, 64, 128, 8, seed=3, mean=(0.2, -0.1))
    P, S = O.Scheme(64, 128, 0.01, 1.3, 0.01, Ly=2 * TWO_PI), F.ForcedScheme(64, 128, 0.01, 1.3, 0.01, Ly=2 * TWO_PI)
    w, mean = P.init(u0, v0)
    assert np.array_equal(S.nonlinear(w, mean), P.nonlinear(w, mean))
    wp, ws = P.step(w, mean, 5), S.step(w, mean, 5)
    assert np.array_equal(wp, ws)
    for a, b in zip(P.fields(wp, mean), S.fields(ws, mean)):
        assert np.array_equal(a, b)
    assert np.array_equal(S.diag(ws)[2], np.zeros(2))
    assert np.array_equal(S.expand(S.compact(ws)), ws)


# ---------------------------------------------------------------------------------------------------- analytic solutions
@pytest.mark.parametrize('nx,ny,Ly', [(64, 128, TWO_PI), (128, 64, 2 * TWO_PI)])
@pytest.mark.parametrize('drag', [0.0, 0.5])
@pytest.mark.parametrize('U0', [0.0, 0.7])
def test_laminar_kolmogorov_flow_from_rest(nx, ny, Ly, drag, U0):
    # f = (A sin(k y), 0) from u = (U0, 0): w depends on y alone and v = 0, so u w_x + v w_y = 0 identically and each mode obeys
    # w' = -lam w + g.  The integrating factor turns that into the quadrature of exp(lam s) g, which RK4 does by Simpson's rule: local error
    # (lam dt)^5 / 2880 per step relative to the forced amplitude A / lam, at most n times that after n steps.  Bound: 10x over it (plus
    # 1e-13 for rounding).  lam dt = 0.08 (Ly = 2 pi), 0.02 (Ly = 4 pi), + 0.05 with the drag; measured error over n local errors in the
    # 8 cases: 0.36 .. 0.82, i.e. max|u - u_exact| lam / A from 1.8e-11 (lam dt = 0.02) to 9.2e-8 (lam dt = 0.13); U0 changes nothing.
    # The force is the exact float64 sine here: rounded to float32, as the device gets it, it alone moves u by 2e-9 of the amplitude
    k, A, nu, dt, n = 4, 1.5, 0.05, 0.1, 20
    lam = nu * (TWO_PI * k / Ly) ** 2 + drag
    S = F.ForcedScheme(nx, ny, dt, 1.0, nu, Ly=Ly, drag=drag).kolmogorov_forcing(k, A, dtype=np.float64)
    got = run(S, np.full((nx, ny), U0), np.zeros((nx, ny)), n)
    ref = F.kolmogorov_laminar(nx, ny, n * dt, A, k, lam, Ly, U0)
    local = (lam * dt) ** 5 / 2880
    err = np.abs(got[0] - ref[0]).max() * lam / A
    print('laminar Kolmogorov %dx%d Ly %.3g drag %g U0 %g: lam dt %.3g, error / amplitude %.2e = %.2f x n local errors'
          % (nx, ny, Ly, drag, U0, lam * dt, err, err / (n * local)))
    assert err <= 10 * n * local + 1e-13, (err, n * local)
    assert np.abs(got[1]).max() <= 1e-13 and np.abs(got[2]).max() <= 1e-13
    # and the force does act: without it the flow stays at rest
    assert np.abs(ref[0] - U0).max() >= 0.5 * A / lam * (1 - math.exp(-lam * n * dt))


@pytest.mark.parametrize('nx,ny,Ly', [(64, 64, TWO_PI), (64, 256, 2 * TWO_PI)])
@pytest.mark.parametrize('dt', [0.01, 0.1, 0.5])
def test_taylor_green_with_drag_is_reproduced_at_any_dt(nx, ny, Ly, dt):
    # J(psi, w) = 0 for Taylor-Green and the drag is part of the integrating factor: exact decay exp(-(2 nu + alpha) t) at any dt
    nu, rho, n, alpha = 0.05, 1.3, 10, 0.3
    S = F.ForcedScheme(nx, ny, dt, rho, nu, Ly=Ly, drag=alpha)
    u0, v0, _ = O.taylor_green(nx, ny, 0.0, nu, rho, Ly=Ly)
    got = run(S, u0, v0, n)
    u, v, p = O.taylor_green(nx, ny, n * dt, nu, rho, Ly=Ly)
    d = math.exp(-alpha * n * dt)
    for g, r in zip(got, (u * d, v * d, p * d * d)):
        assert np.abs(g - r).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------- diagnostics
def _budget_error(dt, t, u0, v0):
    nu, alpha = 0.01, 0.1
    S = F.ForcedScheme(64, 64, dt, 1.0, nu, drag=alpha).kolmogorov_forcing(4, 1.0)
    w, mean = S.init(u0, v0)
    n = int(round(t / dt))
    wm = S.step(w, mean, n - 1)
    w0 = S.step(wm, mean, 1)
    wp = S.step(w0, mean, 1)
    E, Z, P = S.diag(w0)
    lhs = (S.diag(wp)[0] - S.diag(wm)[0]) / (2 * dt)
    rhs = P - 2 * nu * Z - 2 * alpha * E
    return float(np.abs(lhs - rhs).max()), float(np.abs(rhs).max()), float(np.abs(P).max())


def test_energy_budget_closes_at_second_order_of_the_centred_difference():
    # dE/dt = P - 2 nu Z - 2 alpha E at t = 0.4 from a random |m| <= 8 start (max|u| = 1) under Kolmogorov forcing (k = 4, A = 1) and drag
    # 0.1: the centred difference of E is second order in dt (the scheme's own error is fourth order), so halving dt quarters the
    # mismatch.  Measured: |lhs - rhs| 3.22e-5 at dt = 0.02, 8.06e-6 at 0.01, ratio 4.000 (|rhs| 0.125, P 0.171)
    u0, v0 = O.random_ic(2, 64, 64, 8, seed=6, umax=1.0, mean=(0.3, -0.2))
    e1, rhs, P = _budget_error(0.02, 0.4, u0, v0)
    e2, _, _ = _budget_error(0.01, 0.4, u0, v0)
    print('energy budget: |dE/dt - (P - 2 nu Z - 2 alpha E)| %.3e (dt 0.02) %.3e (dt 0.01) ratio %.3f; |rhs| %.3e, P %.3e' % (e1, e2, e1 / e2, rhs, P))
    assert 3.5 <= e1 / e2 <= 4.5, (e1, e2)
    assert P > 1e-3 and e1 <= 1e-2 * rhs                       # the force does work, and the budget closes


def test_diag_matches_the_physical_space_definitions():
    S = F.ForcedScheme(64, 128, 0.01, 1.0, 0.01, Lx=3.0, Ly=5.0, drag=0.2)
    fx, fy = FC.random_forces(3, 64, 128, 8, 3.0, 5.0)
    S.set_forcing(fx, fy)
    u0, v0 = O.band_ic(3, 64, 128, 4, 3.0, 5.0, mean=(0.4, -0.3))
    w, mean = S.init(u0, v0)
    w = S.step(w, mean, 5)
    E, Z, P = S.diag(w)
    u, v, _ = S.fields(w, mean)
    up, vp = u - mean[:, 0, None, None], v - mean[:, 1, None, None]
    E_phys = 0.5 * (up * up + vp * vp).mean(axis=(-2, -1))
    fsx, fsy = S.forcing_fields()
    P_phys = (fsx * u + fsy * v).mean(axis=(-2, -1))
    assert np.abs(E / E_phys - 1).max() <= 1e-12
    assert np.abs(Z / S.enstrophy(w) - 1).max() <= 1e-12
    assert np.abs(P - P_phys).max() <= 1e-12 * np.abs(P_phys).max()
    assert np.abs(S.energy(w, mean) - (E + 0.5 * (mean ** 2).sum(axis=-1))).max() <= 1e-12 * E.max()
    # f_s is solenoidal, zero-mean, band-limited, and here (a force that already is all three) the force itself
    assert np.abs(S.divergence(fsx, fsy)).max() <= 1e-10 * np.abs(fsx).max()
    assert np.abs(fsx - fx).max() <= 1e-6 * np.abs(fx).max() and np.abs(fsy - fy).max() <= 1e-6 * np.abs(fy).max()      # float32 inputs


def test_forcing_fields_project_a_rough_force():
    nx, ny = 64, 128
    S = F.ForcedScheme(nx, ny, 0.01, 1.0, 0.01)
    fx, fy = FC.rough_force(nx, ny, 5)
    S.set_forcing(fx, fy)
    fsx, fsy = S.forcing_fields()
    assert fsx.shape == (1, nx, ny)
    assert abs(fsx.mean()) <= 1e-14 and abs(fsy.mean()) <= 1e-14
    assert np.abs(S.divergence(fsx, fsy)).max() <= 1e-12 * nx
    outside = 1 - S.M
    assert np.linalg.norm(np.fft.rfft2(fsx) * outside) <= 1e-12 * np.linalg.norm(np.fft.rfft2(fsx))
    assert rel_l2(fsx, fx.astype(np.float64)) > 0.1             # the projection removed a real part of it
    # the vorticity equation sees the same force: g^ of f_s is g^ of f
    g2 = S.init(fsx, fsy)[0]
    assert np.abs(g2 - S.g).max() <= 1e-12 * np.abs(S.g).max()


def test_fourth_order_in_time_with_force_and_drag():
    # the set-up of test_oracle_pspec.py::test_fourth_order_in_time plus a Kolmogorov force (k = 4, A = 2) and drag 0.5: measured ratios
    # 16.25 and 16.16 (errors 1.9e-5, 1.2e-6, 7.1e-8)
    u0, v0 = O.random_ic(1, 64, 64, 4, seed=1, umax=2.0)
    mk = lambda n: F.ForcedScheme(64, 64, 0.5 / n, 1.0, 0.01, drag=0.5).kolmogorov_forcing(4, 2.0)
    ref = run(mk(640), u0, v0, 640)
    errs = []
    for n in (10, 20, 40):
        got = run(mk(n), u0, v0, n)
        errs.append(max(rel_l2(g, r) for g, r in zip(got[:2], ref[:2])))
    print('forced 4th order: errors %s ratios %s' % (['%.2e' % e for e in errs], ['%.2f' % (a / b) for a, b in zip(errs, errs[1:])]))
    for a, b in zip(errs, errs[1:]):
        assert 12 <= a / b <= 20, errs


# ---------------------------------------------------------------------------------------------------- the GPU cases can tell
REDUCED = sorted(set((min(c[0], 256), min(c[1], 256), 1, c[3], c[4], c[5]) for c in C.FULL_BAND))


@pytest.mark.parametrize('case', REDUCED, ids=[C.case_id(c) + '_L%.3g' % c[3] for c in REDUCED])
def test_forced_cases_detect_an_ignored_force_drag_or_stage(case):
    # the GPU cases of tests/test_gpu_pspec_forced.py (axes cut to <= 256, B = 1): a build that ignores g^, ignores the drag, or adds g^ in
    # stage 1 only moves the velocity by >= 100x the GPU bound BOUND_UV (2e-6).  Measured here, the larger of u and v over these cases:
    # no force 8.3e-2 .. 7.6e-1, no drag 1.3e-2 .. 8.6e-2, stage 1 only 6.9e-2 .. 6.4e-1
    nx, ny, B, Lx, Ly, mean = case
    u0, v0, dt = C.full_band_input(*case)
    _, ref = FC.oracle_run(FC.scheme(nx, ny, dt, Lx, Ly).kolmogorov_forcing(FC.KF, FC.AMP), u0, v0)
    variants = dict(no_force=FC.scheme(nx, ny, dt, Lx, Ly), no_drag=FC.scheme(nx, ny, dt, Lx, Ly, drag=0.0).kolmogorov_forcing(FC.KF, FC.AMP),
                    stage_1_only=FC.scheme(nx, ny, dt, Lx, Ly, force_stages=(1,)).kolmogorov_forcing(FC.KF, FC.AMP))
    sep = {}
    for name, S in variants.items():
        _, got = FC.oracle_run(S, u0, v0)
        sep[name] = max(rel_l2(g, r) for g, r in zip(got[:2], ref[:2]))
    print('%dx%d L %.3g x %.3g separations (rel-L2, larger of u, v): %s' % (nx, ny, Lx, Ly, {k: '%.1e' % v for k, v in sep.items()}))
    for name in sep:
        assert sep[name] >= 100 * C.BOUND_UV, (name, sep)
    # the unforced parent scheme is the no-force, no-drag variant: further away still
    _, plain = C.oracle_run(u0, v0, dt, nx, ny, Lx, Ly)
    assert max(rel_l2(g, r) for g, r in zip(plain[:2], ref[:2])) >= 100 * C.BOUND_UV


# ---------------------------------------------------------------------------------------------------- host argument checks
def _solver(**kw):
    from nns.periodic import PeriodicSolver
    args = dict(nx=64, ny=64, dt=0.01, rho=1.0, nu=0.01)
    args.update(kw)
    return PeriodicSolver(**args)


@pytest.mark.parametrize('kw,exc', [
    (dict(drag=-0.1), ValueError), (dict(drag=math.inf), ValueError), (dict(drag=math.nan), ValueError), (dict(drag='0.1'), TypeError),
    (dict(drag=True), TypeError), (dict(drag=None), TypeError)])
def test_solver_rejects_a_bad_drag(kw, exc):
    with pytest.raises(exc):
        _solver(**kw)


def test_forcing_calls_are_checked_before_any_device_use():
    s = _solver(nx=64, ny=128, drag=0.25)
    assert s.drag == 0.25 and s.ghat is None and _solver().drag == 0.0
    f64 = np.zeros((64, 128))
    f32 = np.zeros((64, 128), dtype=np.float32)
    with pytest.raises(TypeError):
        s.set_forcing(f64, f64)
    with pytest.raises(TypeError):
        s.set_forcing(f32, [[0.0]])
    with pytest.raises(TypeError):
        s.set_forcing(f32)
    with pytest.raises(ValueError):
        s.set_forcing(f32.T.copy(), f32.T.copy())
    with pytest.raises(ValueError):
        s.set_forcing(np.zeros((2, 2, 64, 128), dtype=np.float32), np.zeros((2, 2, 64, 128), dtype=np.float32))
    with pytest.raises(ValueError):
        s.set_forcing(np.zeros((2, 64, 128), dtype=np.float32), f32)
    with pytest.raises(ValueError):
        s.set_forcing(None, f32)
    for k in (0, -4, 43, 64):                                   # ny = 128 keeps m_y <= 42
        with pytest.raises(ValueError):
            s.kolmogorov_forcing(k=k)
    with pytest.raises(TypeError):
        s.kolmogorov_forcing(k=4.0)
    with pytest.raises(TypeError):
        s.kolmogorov_forcing(k=4, amplitude='1')
    with pytest.raises(ValueError):
        s.kolmogorov_forcing(k=4, amplitude=math.inf)
    assert s.set_forcing(None) is s and s.ghat is None and s.forcing_fields() is None
    with pytest.raises(TypeError):
        s.diagnostics(None)
