"""CPU checks of the passive-scalar restatement (tests/pspec_scalar_oracle.py) that the GPU solver's scalar step and diagnostics
(csrc/pspec_kernels.hip: nns_spec_ns_step_scalar_f32, nns_spec_ns_scalar_*) are compared against: it leaves the flow alone, obeys the mean
law and the variance budget, reproduces the advected sine, and the bound of tests/test_gpu_pspec_scalar.py would catch each of its wrong
variants; and of PeriodicSolver's argument checks for the scalar (raised before any device use)."""
import os
import re

import numpy as np
import pytest

import pspec_cases as C
import pspec_forced_cases as FC
import pspec_scalar_cases as SC
import pspec_scalar_oracle as SO
from conftest import ROOT

SCALAR_SYMBOLS = ['nns_spec_ns_scalar_diag_f32', 'nns_spec_ns_scalar_field_f32', 'nns_spec_ns_scalar_init_f32', 'nns_spec_ns_scalar_workspace',
                  'nns_spec_ns_step_scalar_f32']
IDS = [C.case_id(c) for c in SC.CASES]

reference = SC.reference


# ---------------------------------------------------------------------------------------------------- 1. the interface exists
def test_the_scalar_entry_points_are_declared_and_bound():
    from nns import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nns.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(nns_[a-z0-9_]+)\s*\(', txt))
    for name in SCALAR_SYMBOLS:
        assert name in declared, name
        assert name in _lib.exported_names(), name
    # the step takes what, that, mean, ghat | gbatch | work | work_bytes | batch, nx, ny | Lx, Ly, dt, nu, drag, kappa, gx, gy | nsteps | stream
    assert len(_lib._SINGLE['nns_spec_ns_step_scalar_f32']) == 20
    from nns import ops, periodic
    for f in ('spec_ns_scalar_workspace', 'spec_ns_scalar_init', 'spec_ns_scalar_field', 'spec_ns_step_scalar_', 'spec_ns_scalar_diag'):
        assert callable(getattr(ops, f)), f
    assert periodic.ScalarDiagnostics._fields == ('variance', 'dissipation', 'flux_x', 'flux_y')


def test_solver_argument_checks_for_the_scalar():
    from nns.periodic import PeriodicSolver
    s = PeriodicSolver(64, 64, 0.01, 1.0, 0.01)
    assert s.kappa is None and s.scalar_gradient == (0.0, 0.0)
    s = PeriodicSolver(64, 64, 0.01, 1.0, 0.01, kappa=0, scalar_gradient=(1, -2.5))
    assert s.kappa == 0.0 and s.scalar_gradient == (1.0, -2.5)
    for bad in (-1e-3, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            PeriodicSolver(64, 64, 0.01, 1.0, 0.01, kappa=bad)
    for bad in ('0.1', True):
        with pytest.raises(TypeError):
            PeriodicSolver(64, 64, 0.01, 1.0, 0.01, kappa=bad)
    for bad in ((0.0, float('nan')), (float('inf'), 0.0)):
        with pytest.raises(ValueError):
            PeriodicSolver(64, 64, 0.01, 1.0, 0.01, kappa=0.1, scalar_gradient=bad)
    for bad in (1.0, (1.0,), (1.0, 2.0, 3.0), ('a', 0.0), (True, 0.0)):
        with pytest.raises(TypeError):
            PeriodicSolver(64, 64, 0.01, 1.0, 0.01, kappa=0.1, scalar_gradient=bad)
    z = np.zeros((64, 64), dtype=np.float32)
    with pytest.raises(ValueError, match='kappa'):
        PeriodicSolver(64, 64, 0.01, 1.0, 0.01).init(z, z, theta=z)                 # refused before any device use
    s = PeriodicSolver(64, 64, 0.01, 1.0, 0.01, kappa=0.1)
    with pytest.raises(TypeError):
        s.init(z, z, theta=z.astype(np.float64))
    with pytest.raises(ValueError):
        s.init(z, z, theta=np.zeros((64, 128), dtype=np.float32))
    with pytest.raises(ValueError):
        s.init(z, z, theta=np.zeros((2, 64, 64), dtype=np.float32))


# ---------------------------------------------------------------------------------------------------- 2. the flow is left alone
@pytest.mark.parametrize('case', SC.CASES, ids=IDS)
def test_the_flow_is_the_forced_scheme_s_exactly(case):
    S, u0, v0, th0, w, t, mean = reference(case)
    nx, ny, B, Lx, Ly, _ = case
    P = FC.scheme(nx, ny, S.dt, Lx, Ly).kolmogorov_forcing(FC.KF, FC.AMP)
    wp, _ = FC.oracle_run(P, u0, v0, SC.NSTEPS)
    assert np.array_equal(w, wp)
    assert np.abs(w).max() > 0 and np.abs(S.fluctuation(t)).max() > 0


# ---------------------------------------------------------------------------------------------------- 3. the mean law
@pytest.mark.parametrize('case', SC.CASES, ids=IDS)
def test_the_mean_of_the_scalar_follows_the_mean_flow_down_the_gradient(case):
    # d<theta>/dt = -G . (U0, V0): the (0, 0) mode of u theta_x + v theta_y is alias-free (a sum over k of u^(k) conj(i k theta^(k)), inside
    # the band) and zero because div u = 0
    S, u0, v0, th0, w, t, mean = reference(case)
    n = case[0] * case[1]
    mean0 = S.init_scalar(th0)[..., 0, 0].real / n
    want = mean0 - SC.NSTEPS * S.dt * (SC.GRAD[0] * mean[..., 0] + SC.GRAD[1] * mean[..., 1])
    err = np.abs(t[..., 0, 0].real / n - want).max()
    print('%s: mean of theta %s, G . U dt n = %s, error %.2e' % (C.case_id(case), t[..., 0, 0].real / n, want - mean0, err))
    assert err <= 1e-9, err
    assert np.abs(t[..., 0, 0].imag).max() <= 1e-9 * n


# ---------------------------------------------------------------------------------------------------- 4. the variance budget
@pytest.mark.parametrize('case', SC.CASES, ids=IDS)
def test_the_variance_budget_closes_at_the_second_order_of_a_centred_difference(case):
    # d/dt 1/2 <theta'^2> = -G . <u theta'> - kappa <|grad theta|^2>: the centred difference of the variance over steps 5 and 7 against the
    # right-hand side at step 6, relative to |G . flux| + dissipation.  Bound 2e-3: the O(dt^2) of the difference (measured 3e-5 .. 8e-4)
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0 = reference(case)[:4]
    w, mean = S.init(u0, v0)
    t = S.init_scalar(th0)
    w, t = S.step(w, t, mean, 5)
    d5 = S.scalar_diag(w, t)
    w, t = S.step(w, t, mean, 1)
    d6 = S.scalar_diag(w, t)
    w, t = S.step(w, t, mean, 1)
    d7 = S.scalar_diag(w, t)
    lhs = (d7[0] - d5[0]) / (2 * S.dt)
    gflux = SC.GRAD[0] * d6[2] + SC.GRAD[1] * d6[3]
    err = np.abs(lhs + gflux + d6[1]) / (np.abs(gflux) + d6[1])
    print('%s: d var / dt %s, -G . flux %s, -dissipation %s, relative closure %s' % (C.case_id(case), lhs, -gflux, -d6[1], err))
    assert err.max() <= 2e-3, err
    # and the diagnostics are the grid averages they claim to be
    th, (u, v, _) = S.scalar_field(t), S.fields(w, mean)
    tp = th - th.mean(axis=(-2, -1), keepdims=True)
    gx, gy = S.irfft2(1j * S.kx * t), S.irfft2(1j * S.ky * t)
    direct = (0.5 * (tp ** 2).mean(axis=(-2, -1)), S.kappa * (gx ** 2 + gy ** 2).mean(axis=(-2, -1)), (u * tp).mean(axis=(-2, -1)),
              (v * tp).mean(axis=(-2, -1)))
    for a, b in zip(d7, direct):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


# ---------------------------------------------------------------------------------------------------- 5. the advected sine
@pytest.mark.parametrize('sine', SC.SINES, ids=['%dx%d' % s[:2] for s in SC.SINES])
def test_advected_sine_under_a_uniform_flow(sine):
    # w = 0 and means (U0, V0): theta = sin(k . (x - U t)) exp(-kappa |k|^2 t) + c - t G . U.  The diffusion is exact in the integrating factor
    # and the advection of one mode is theta^' = -i omega theta^, omega = k . U, which RK4 integrates with n (omega dt)^5 / 120 of the amplitude:
    # predicted 4.0e-8, 2e-8, 1e-8 for the three cases.  Bound 1e-7 of the decayed amplitude, which stays >= 0.5
    nx, ny, Lx, Ly, m, U, kappa, dt = sine
    n = SC.SINE_STEPS
    S = SO.ScalarScheme(nx, ny, dt, 1.0, 0.01, Lx, Ly, kappa=kappa, grad=SC.SINE_GRAD)
    w, mean = S.init(np.full((nx, ny), U[0]), np.full((nx, ny), U[1]))
    th0, _ = SO.advected_sine(nx, ny, 0.0, m, U, kappa, SC.SINE_GRAD, SC.SINE_MEAN, Lx, Ly)
    w, t = S.step(w, S.init_scalar(th0), mean, n)
    ref, amp = SO.advected_sine(nx, ny, n * dt, m, U, kappa, SC.SINE_GRAD, SC.SINE_MEAN, Lx, Ly)
    err = np.abs(S.scalar_field(t) - ref).max() / amp
    omega = 2 * np.pi * (m[0] * U[0] / Lx + m[1] * U[1] / Ly)
    print('advected sine %dx%d m %s: error / amplitude %.2e, predicted %.2e, amplitude %.3f' % (nx, ny, m, err, n * abs(omega * dt) ** 5 / 120, amp))
    assert np.abs(w).max() == 0.0
    assert amp >= 0.5 and err <= 1e-7, (err, amp)


# ---------------------------------------------------------------------------------------------------- 6. wrong schemes are caught
def _distance(case, **kw):
    """rel-L2 of a wrong scheme's fluctuation spectrum against the correct one's, after the case's 12 steps."""
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0, w, t, mean = reference(case)
    _, tm, _ = SC.oracle_run(SC.scheme(nx, ny, S.dt, Lx, Ly, **kw), u0, v0, th0)
    return SC.rel_l2c(S.fluctuation(tm), S.fluctuation(t))


@pytest.mark.parametrize('case', SC.CASES, ids=IDS)
def test_cases_detect_a_wrong_diffusivity_an_ignored_gradient_and_a_dragged_scalar(case):
    # the GPU test bounds the fluctuation spectrum by C.BOUND_W: each of these is >= 100x that away on every case
    d = {m: _distance(case, mutate=m) for m in ('nokappa', 'nograd', 'kappa_is_nu', 'dragged')}
    print('%s: distance of the wrong schemes / BOUND_W: %s' % (C.case_id(case), {m: '%.0f' % (e / C.BOUND_W) for m, e in d.items()}))
    assert min(d.values()) >= 100 * C.BOUND_W, d


@pytest.mark.parametrize('case', SC.CASES, ids=IDS)
def test_cases_detect_a_frozen_velocity_and_a_mask_one_mode_too_wide(case):
    # asserted at 64 x 64; along a 1024-long axis these are as small as 7e-6, so on the other cases they are only printed
    d = {'frozen': _distance(case, mutate='frozen'), 'widen x': _distance(case, widen=(1, 0)), 'widen y': _distance(case, widen=(0, 1))}
    print('%s: distance of the wrong schemes / BOUND_W: %s' % (C.case_id(case), {m: '%.1f' % (e / C.BOUND_W) for m, e in d.items()}))
    if case[:2] == (64, 64):
        assert min(d.values()) >= 100 * C.BOUND_W, d
