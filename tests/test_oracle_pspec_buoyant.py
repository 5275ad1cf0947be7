"""CPU checks of the float64 restatement of the Boussinesq buoyancy (tests/pspec_buoyant_oracle.py): it is the passive scheme at b = 0, it
reproduces the analytic plane waves at RK4's order, its energy budgets close, its buoyancy spectrum and pressure are consistent, and the bounds
of tests/test_gpu_pspec_buoyant.py would catch each of its mutations."""
import numpy as np
import pytest

import pspec_buoyant_cases as BC
import pspec_buoyant_oracle as BO
import pspec_cases as C
import pspec_scalar_cases as SC
import pspec_scalar_oracle as SO

CASE = BC.CASES[0]                      # 64 x 64, B = 3, with a mean flow


def inputs(case=CASE):
    u0, v0, dt = C.full_band_input(*case)
    return u0, v0, SC.scalar_input(*case), dt


# ---------------------------------------------------------------------------------------------------- the passive scheme at b = 0
@pytest.mark.parametrize('forced', [False, True], ids=['unforced', 'forced'])
def test_zero_buoyancy_is_the_passive_scheme_bit_for_bit(forced):
    nx, ny, B, Lx, Ly, _ = CASE
    u0, v0, th0, dt = inputs()
    P = SC.scheme(nx, ny, dt, Lx, Ly, forced)
    Z = BC.scheme(nx, ny, dt, Lx, Ly, forced, buoy=(0.0, 0.0))
    w, mean = P.init(u0, v0)
    t = P.init_scalar(th0)
    pw, pt = P.step(w, t, mean, 3)
    zw, zt = Z.step(w, t, mean, 3)
    assert np.array_equal(pw, zw) and np.array_equal(pt, zt)
    bw, _ = BC.scheme(nx, ny, dt, Lx, Ly, forced).step(w, t, mean, 3)
    assert not np.array_equal(bw, pw)
    for a, b in zip(Z.fields(zw, mean, zt), P.fields(pw, mean)):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- plane waves
def wave_error(wave, U, nsteps, dt):
    """max error of w and of theta's fluctuation after nsteps steps, each over its decayed or grown amplitude."""
    nx, ny, Lx, Ly, m, b, G, nu, _ = wave
    S = BO.BuoyantScheme(nx, ny, dt, C.RHO, nu, Lx, Ly, kappa=nu, grad=G, buoy=b)
    u0, v0, _, th0 = BO.plane_wave(nx, ny, 0.0, m, b, G, U, nu, Lx, Ly)[:4]
    w, mean = S.init(u0, v0)
    w, t = S.step(w, S.init_scalar(th0), mean, nsteps)
    _, _, rw, rt, aw, at, om = BO.plane_wave(nx, ny, nsteps * dt, m, b, G, U, nu, Lx, Ly)
    th = S.scalar_field(t)
    ew = np.abs(S.irfft2(w) - rw).max() / aw
    et = np.abs((th - th.mean()) - (rt - rt.mean())).max() / at
    return ew, et, np.abs(th.mean() - rt.mean())


@pytest.mark.parametrize('wave', [BC.WAVES[0], BC.WAVES[3]], ids=[BC.WAVE_IDS[0], BC.WAVE_IDS[3]])
def test_plane_wave_without_a_mean_flow_has_rk4s_error_and_order(wave):
    # a 2 x 2 linear system with eigenvalues +- i omega (+- omega when unstable) under the exact decay: RK4 drops the (omega dt)^5 / 120 term of the
    # exponential every step, n (omega dt)^5 / 120 of the amplitude after n steps; 9.4e-11 here, and 16x less per halving of dt
    dt = wave[8]
    pred = BC.wave_rk4_error(wave, (0.0, 0.0))
    e1 = max(wave_error(wave, (0.0, 0.0), BC.WAVE_STEPS, dt)[:2])
    e2 = max(wave_error(wave, (0.0, 0.0), 2 * BC.WAVE_STEPS, dt / 2)[:2])
    print('plane wave %dx%d b %s G %s, no mean flow: error %.3e (predicted %.3e), at dt / 2 %.3e, ratio %.2f' % (wave[0], wave[1], wave[5], wave[6], e1, pred, e2, e1 / e2))
    assert 0.9 * pred <= e1 <= 1.1 * pred, (e1, pred)
    assert 15.0 <= e1 / e2 <= 17.0, e1 / e2


@pytest.mark.parametrize('wave', BC.WAVES, ids=BC.WAVE_IDS)
def test_plane_wave_under_its_mean_flow_200_steps(wave):
    # the wave is also carried by U (G . U = 0): the eigenvalues move to -i k . U +- i omega, so the error is <= n ((omega + |k . U|) dt)^5 / 120
    U = BC.wave_flow(wave[6])
    pred = BC.wave_rk4_error(wave, U)
    ew, et, em = wave_error(wave, U, BC.WAVE_STEPS, wave[8])
    print('plane wave %dx%d m %s under U = (%.3f, %.3f): errors %.3e (w), %.3e (theta\') of the amplitudes, bound %.3e; mean of theta off by %.1e'
          % (wave[0], wave[1], wave[4], U[0], U[1], ew, et, pred, em))
    assert max(ew, et) <= pred <= 7.2e-8, (ew, et, pred)
    assert em <= 1e-13


# ---------------------------------------------------------------------------------------------------- budgets
def budget_gap(S, w, t, mean, k):
    """|dE/dt by a centred difference over steps k - 1, k + 1 - (P - 2 nu Z - 2 alpha E + b . flux) at step k| and the buoyancy term there."""
    w, t = S.step(w, t, mean, k - 1)
    e0 = S.diag(w)[0]
    w, t = S.step(w, t, mean, 1)
    E, Z, P = S.diag(w)
    bp = S.buoyancy_power(w, t)
    w2, _ = S.step(w, t, mean, 1)
    lhs = (S.diag(w2)[0] - e0) / (2 * S.dt)
    return np.abs(lhs - (P - 2 * S.nu * Z - 2 * S.drag * E + bp)), np.abs(bp)


def test_energy_budget_closes_at_second_order_in_dt():
    # the centred difference is the only O(dt^2) term: the gap falls 4x per halving of dt at the same time t = 2 dt
    nx, ny, B, Lx, Ly, _ = CASE
    u0, v0, th0, dt = inputs()
    gaps = []
    for h, k in ((dt, 2), (dt / 2, 4), (dt / 4, 8)):
        S = BC.scheme(nx, ny, h, Lx, Ly)
        w, mean = S.init(u0, v0)
        gaps.append(budget_gap(S, w, S.init_scalar(th0), mean, k))
    (g1, bp), (g2, _), (g3, _) = gaps
    print('energy budget 64x64: gap / buoyancy term %s at dt, ratios %s and %s per halving' % (g1 / bp, g1 / g2, g2 / g3))
    assert np.all(bp > 0) and np.all(g1 <= 0.05 * bp), (g1, bp)
    assert np.all(np.abs(g1 / g2 - 4.0) <= 0.1) and np.all(np.abs(g2 / g3 - 4.0) <= 0.1), (g1 / g2, g2 / g3)


def test_aligned_buoyancy_conserves_energy_plus_variance():
    # b = lambda G, nu = kappa = alpha = 0, no force: dE/dt = lambda G . flux = -lambda d variance / dt.  The Galerkin truncation conserves the
    # quadratic invariant exactly, so what drifts is RK4's own amplitude error, (omega dt)^6 / 144 per step and mode: at the full-band case's
    # dt (CFL 0.5) 3.6e-7 over 200 steps, at a quarter of it 4^6 = 4096x less, 9e-11, which is where 1e-9 can be asked
    nx, ny, B, Lx, Ly, _ = CASE
    u0, v0, th0, dt = inputs()
    dt = dt / 4
    lam = 1.5
    G = BC.GRAD
    S = BO.BuoyantScheme(nx, ny, dt, C.RHO, 0.0, Lx, Ly, kappa=0.0, grad=G, buoy=(lam * G[0], lam * G[1]))
    w, mean = S.init(u0, v0)
    t = S.init_scalar(th0)
    total = lambda w, t: S.diag(w)[0] + lam * S.scalar_diag(w, t)[0]
    c0, e0 = total(w, t), S.diag(w)[0]
    w, t = S.step(w, t, mean, 200)
    c1, e1 = total(w, t), S.diag(w)[0]
    print('E + lambda variance: %s -> drift %s relative; E alone moved by %s relative' % (c0, np.abs(c1 / c0 - 1), np.abs(e1 / e0 - 1)))
    assert np.abs(c1 / c0 - 1).max() <= 1e-9
    assert np.abs(e1 / e0 - 1).min() >= 1e-3                      # the exchange is there: E alone is not conserved


# ---------------------------------------------------------------------------------------------------- spectrum and pressure
def test_buoyancy_spectrum_sums_to_the_power_and_the_pressure_solves_its_poisson_equation():
    S, u0, v0, th0, w, t, mean = BC.reference(CASE)
    bs, bp = S.buoyancy_spectrum(w, t), S.buoyancy_power(w, t)
    assert bs.shape[:-1] == bp.shape and np.all(np.abs(bp) > 0)
    assert np.abs(bs.sum(axis=-1) / bp - 1).max() <= 1e-13
    r = S.poisson_residual(w, mean, t)
    print('buoyant pressure: Poisson residual %.2e of the source' % r)
    assert r <= 1e-10
    # u, v are the parent's and p differs from it by the buoyancy's part
    u, v, p = S.fields(w, mean, t)
    pu, pv, pp = SO.ScalarScheme.fields(S, w, mean)
    assert np.array_equal(u, pu) and np.array_equal(v, pv) and SC.rel_l2c(p, pp) > 0.1


# ---------------------------------------------------------------------------------------------------- mutations
@pytest.mark.parametrize('mutate', ['sign', 'swap', 'none', 'frozen'])
def test_the_state_bound_catches_every_mutation_of_the_step(mutate):
    # measured: 'sign' 5.0e-2, 'swap' 2.5e-2, 'none' 2.5e-2, 'frozen' 3.5e-4 against BOUND_W = 2e-6
    nx, ny, B, Lx, Ly, _ = CASE
    S, u0, v0, th0, w, t, mean = BC.reference(CASE)
    mw, mt, _ = BC.oracle_run(BC.scheme(nx, ny, S.dt, Lx, Ly, mutate=mutate), u0, v0, th0)
    e = SC.rel_l2c(S.compact(mw), S.compact(w))
    print('mutation %s: what moves by %.2e rel-L2 (%.0fx BOUND_W)' % (mutate, e, e / C.BOUND_W))
    assert e >= 100 * C.BOUND_W, e


def test_the_pressure_bound_catches_a_pressure_without_buoyancy():
    nx, ny, B, Lx, Ly, _ = CASE
    S, u0, v0, th0, w, t, mean = BC.reference(CASE)
    M = BC.scheme(nx, ny, S.dt, Lx, Ly, mutate='p_without_b')
    e = SC.rel_l2c(M.fields(w, mean, t)[2], S.fields(w, mean, t)[2])
    print("mutation p_without_b: p moves by %.2e rel-L2 (%.0fx BC.BOUND_P)" % (e, e / BC.BOUND_P))
    assert e >= 100 * BC.BOUND_P, e
