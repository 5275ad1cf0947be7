"""CPU checks of the reverse-mode restatement (tests/pspec_scalar_adjoint_oracle.py) that the GPU adjoint of the periodic solver's scalar and
buoyant step (csrc/pspec_kernels.hip: nns_spec_ns_step_scalar_adjoint_f32, through nns.periodic.PeriodicSolver.advance_scalar) is compared
against: the dot-product identity against central differences of BuoyantScheme.step, the transpose of the linearised nonlinear terms, the
analytic gradient of a fluid at rest, and the distance of every deliberately wrong scheme from the right gradient on the inputs of the GPU
test.  One test needs the package and its binding, not the GPU: the entry points exist."""
import numpy as np
import pytest

import pspec_oracle as O
import pspec_scalar_adjoint_cases as AC
import pspec_scalar_adjoint_oracle as A

TWO_PI = 2 * np.pi


def band_field(S, B, seed):
    """A real field whose spectrum fills the kept band (zero mean)."""
    return O.band_ic(B, S.nx, S.ny, seed, S.Lx, S.Ly, 1.0)[0]


def setup(nx, ny, Lx, Ly, buoy=(0.6, 1.5)):
    B = 2
    u0, v0 = O.band_ic(B, nx, ny, 7 + nx + ny, Lx, Ly, 1.0, mean=(0.3, -0.2))
    dt = O.cfl_dt(nx, ny, Lx, Ly, 1.3)
    S = A.ScalarAdjointScheme(nx, ny, dt, 1.0, 1e-3, Lx, Ly, drag=0.2, kappa=2e-3, grad=(0.7, -0.4), buoy=buoy)
    fx, fy = O.band_ic(B, nx, ny, 11, Lx, Ly, 0.5)
    S.set_forcing(fx, fy)
    w, mean = S.init(u0, v0)
    t = S.init_scalar(band_field(S, B, 12) + 0.25)
    return S, w, t, mean


# ---------------------------------------------------------------------------------------------------- 1. the dot-product identity
@pytest.mark.parametrize('nx,ny,Lx,Ly', [(64, 64, TWO_PI, TWO_PI), (64, 128, 3.0, 7.0)])
@pytest.mark.parametrize('nsteps,buoy', [(1, (0.6, 1.5)), (3, (0.6, 1.5)), (3, (0.0, 0.0))])
def test_step_vjp_against_central_differences(nx, ny, Lx, Ly, nsteps, buoy):
    S, w, t, mean = setup(nx, ny, Lx, Ly, buoy)
    lam = np.fft.rfft2(band_field(S, 2, 21))                   # the cotangents of the result; the scalar's has a mean
    mu = np.fft.rfft2(band_field(S, 2, 24) + 0.1)
    dw = np.fft.rfft2(band_field(S, 2, 22))                    # directions of the state; the scalar's has a mean
    dth = np.fft.rfft2(band_field(S, 2, 25) + 0.3)
    dg = np.fft.rfft2(band_field(S, 2, 23))                    # a direction of the source
    wbar, tbar, gbar = S.step_vjp(w, t, mean, lam, mu, nsteps)
    g0 = S.g

    def loss(eps_w, eps_t, eps_g):
        S.g = g0 + eps_g * dg
        ow, ot = S.step(w + eps_w * dw, t + eps_t * dth, mean, nsteps)
        S.g = g0
        return S.pair(ow, lam) + S.pair(ot, mu)

    # the source acts through dt g per step: its step is 1 / (nsteps dt) larger, so that the difference quotient of each direction stands
    # equally far above the rounding of the loss
    central = lambda k: (lambda e: (loss(*(e * np.eye(3)[k])) - loss(*(-e * np.eye(3)[k]))) / (2 * e))
    for got, fd, scale, what in ((S.pair(wbar, dw), central(0), np.abs(w).max() / np.abs(dw).max(), 'w'),
                                 (S.pair(tbar, dth), central(1), np.abs(t).max() / np.abs(dth).max(), 'theta'),
                                 (S.pair(gbar, dg), central(2), np.abs(w).max() / np.abs(dg).max() / (nsteps * S.dt), 'g')):
        ref = fd(1e-6 * scale)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print('%s %dx%d nsteps=%d b=%s: dot-product identity rel %.2e' % (what, nx, ny, nsteps, buoy, err))
        assert err <= 1e-8, (what, err)


def test_nonlinear_vjp_is_the_transpose_of_the_linearised_nonlinear_terms():
    S, w, t, mean = setup(64, 64, TWO_PI, TWO_PI)
    kappa, m = np.fft.rfft2(band_field(S, 2, 31)), np.fft.rfft2(band_field(S, 2, 33) + 0.2)
    dw, dth = np.fft.rfft2(band_field(S, 2, 32)), np.fft.rfft2(band_field(S, 2, 34) + 0.3)
    e = 1e-5 * np.abs(w).max() / np.abs(dw).max()
    both = lambda s: (S.nonlinear_w(w + s * e * dw, t + s * e * dth, mean, 1), S.nonlinear_scalar(w + s * e * dw, t + s * e * dth, mean))
    (pw, pt), (mw, mt) = both(1.0), both(-1.0)
    lhs = S.pair(kappa, (pw - mw) / (2 * e)) + S.pair(m, (pt - mt) / (2 * e))
    rw, rt = S.nonlinear_vjp(w, t, mean, kappa, m)
    rhs = S.pair(rw, dw) + S.pair(rt, dth)
    assert np.abs(lhs - rhs).max() <= 1e-8 * np.abs(lhs).max()


def test_gradient_from_rest_is_the_decayed_projected_cotangent():
    """Fluid at rest, G = 0, b = 0: the scalar only diffuses, thetabar = exp(-kappa |k|^2 n dt) M_theta mu (the mean included)."""
    S = A.ScalarAdjointScheme(64, 64, 0.01, 1.0, 1e-2, drag=0.3, kappa=2e-2)
    rng = np.random.default_rng(9)
    mu = np.fft.rfft2(rng.standard_normal((1, 64, 64)))
    z = np.zeros_like(mu)
    wbar, tbar, gbar = S.step_vjp(z, S.init_scalar(rng.standard_normal((1, 64, 64))), np.zeros((1, 2)), z, mu, 3)
    ref = np.exp(-S.kappa * S.k2 * S.dt * 3) * S.Mt * mu
    assert np.abs(tbar - ref).max() <= 1e-13 * np.abs(ref).max()


def test_without_buoyancy_and_scalar_cotangent_the_flow_adjoint_is_the_parents():
    """b = 0 and mu = 0: wbar and gbar are those of tests/pspec_adjoint_oracle.py and thetabar is exactly zero, whatever G and theta are (theta
    does not reach w without b); with b != 0 it is not."""
    import pspec_adjoint_oracle as PA
    S, w, t, mean = setup(64, 64, TWO_PI, TWO_PI, buoy=(0.0, 0.0))
    P = PA.AdjointScheme(64, 64, S.dt, 1.0, S.nu, drag=S.drag)
    P.g = S.g
    lam = np.fft.rfft2(band_field(S, 2, 21))
    wbar, tbar, gbar = S.step_vjp(w, t, mean, lam, np.zeros_like(lam), 2)
    pw, pg = P.step_vjp(w, mean, lam, 2)
    assert np.abs(wbar - pw).max() <= 1e-12 * np.abs(pw).max() and np.abs(gbar - pg).max() <= 1e-12 * np.abs(pg).max()
    assert np.abs(tbar).max() == 0.0                           # theta does not reach w without b
    S.buoy = (0.6, 1.5)
    assert np.abs(S.step_vjp(w, t, mean, lam, np.zeros_like(lam), 2)[1]).max() > 0


# ---------------------------------------------------------------------------------------------------- 2. wrong schemes on the GPU's inputs
@pytest.mark.parametrize('case', AC.CASES, ids=AC.case_id)
@pytest.mark.parametrize('wrong', A.WRONG)
def test_the_gpu_bound_would_catch_the_wrong_scheme(case, wrong):
    """Every wrong scheme sits >= 10x the GPU bound away from the right gradient in the worst of wbar, thetabar, gbar.  The buoyancy's adjoint
    can only be got wrong where there is buoyancy: those two mutations must be invisible on the passive case."""
    right, got = AC.oracle_gradient(case), AC.oracle_gradient(case, wrong)
    d = [AC.rel(g, r) for g, r in zip(got, right)]
    print('%s %s: wbar %.2e thetabar %.2e gbar %.2e' % ((AC.case_id(case), wrong) + tuple(d)))
    if wrong in ('buoyancy_sign', 'no_buoyancy_adjoint') and case[6] == AC.PASSIVE:
        assert max(d) == 0.0
        return
    assert max(d) >= 10 * AC.BOUND, d


def test_bound_and_measurements():
    assert AC.BOUND < 1e-5
    assert set(AC.MEASURED) == set(AC.case_id(c) for c in AC.CASES)
    worst = max(max(v) for v in AC.MEASURED.values())
    assert 3 * worst <= AC.BOUND <= 7 * worst, (worst, AC.BOUND)


# ---------------------------------------------------------------------------------------------------- 3. the entry points exist
def test_the_solver_and_the_binding_have_the_scalar_adjoint():
    from nns import _lib
    from nns.periodic import PeriodicSolver
    assert callable(getattr(PeriodicSolver, 'advance_scalar')) and callable(getattr(PeriodicSolver, 'advance_velocity_scalar'))
    names = set(_lib.exported_names())
    assert {'nns_spec_ns_scalar_adjoint_workspace', 'nns_spec_ns_step_scalar_adjoint_f32'} <= names
    L = _lib.lib()
    assert L.nns_spec_ns_scalar_adjoint_workspace is not None and L.nns_spec_ns_step_scalar_adjoint_f32 is not None
