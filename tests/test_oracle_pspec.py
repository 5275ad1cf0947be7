"""CPU checks of the pseudo-spectral solver's restatement (tests/pspec_oracle.py) that the GPU solver (csrc/pspec_kernels.hip,
nns.periodic.PeriodicSolver) is compared against, and of PeriodicSolver's argument checks (raised before any device use)."""
import math

import numpy as np
import pytest

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
