"""CPU checks of the reverse-mode restatement (tests/pspec_adjoint_oracle.py) that the GPU adjoint of the periodic solver's step
(csrc/pspec_kernels.hip: nns_spec_ns_step_adjoint_f32, through nns.periodic.PeriodicSolver.advance) is compared against: the dot-product
identity against central differences of ForcedScheme.step, the adjoints of init and of the velocity, and the distance of every deliberately
wrong scheme from the right gradient on the inputs of the GPU test."""
import numpy as np
import pytest

import pspec_adjoint_cases as AC
import pspec_adjoint_oracle as A
import pspec_oracle as O

TWO_PI = 2 * np.pi


def band_field(S, B, seed):
    """A real field whose spectrum fills the kept band (zero mean)."""
    return O.band_ic(B, S.nx, S.ny, seed, S.Lx, S.Ly, 1.0)[0]


def setup(nx, ny, Lx, Ly):
    B = 2
    u0, v0 = O.band_ic(B, nx, ny, 7 + nx + ny, Lx, Ly, 1.0, mean=(0.3, -0.2))
    dt = O.cfl_dt(nx, ny, Lx, Ly, 1.3)
    S = A.AdjointScheme(nx, ny, dt, 1.0, 1e-3, Lx, Ly, drag=0.2)
    fx, fy = O.band_ic(B, nx, ny, 11, Lx, Ly, 0.5)
    S.set_forcing(fx, fy)
    w, mean = S.init(u0, v0)
    return S, w, mean


# ---------------------------------------------------------------------------------------------------- 1. the dot-product identity
@pytest.mark.parametrize('nx,ny,Lx,Ly', [(64, 64, TWO_PI, TWO_PI), (64, 128, 3.0, 7.0)])
@pytest.mark.parametrize('nsteps', [1, 3])
def test_step_vjp_against_central_differences(nx, ny, Lx, Ly, nsteps):
    S, w, mean = setup(nx, ny, Lx, Ly)
    mu = np.fft.rfft2(band_field(S, 2, 21))                    # the cotangent of the result
    dw = np.fft.rfft2(band_field(S, 2, 22))                    # a direction of the state
    dg = np.fft.rfft2(band_field(S, 2, 23))                    # a direction of the source
    wbar, gbar = S.step_vjp(w, mean, mu, nsteps)
    g0 = S.g

    def loss(eps_w, eps_g):
        S.g = g0 + eps_g * dg
        out = S.pair(S.step(w + eps_w * dw, mean, nsteps), mu)
        S.g = g0
        return out

    scale = np.abs(w).max() / np.abs(dw).max()
    for got, fd, what in ((S.pair(wbar, dw), lambda e: (loss(e, 0.0) - loss(-e, 0.0)) / (2 * e), 'w'),
                          (S.pair(gbar, dg), lambda e: (loss(0.0, e) - loss(0.0, -e)) / (2 * e), 'g')):
        ref = fd(1e-5 * scale)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print('%s %dx%d nsteps=%d: dot-product identity rel %.2e' % (what, nx, ny, nsteps, err))
        assert err <= 1e-7, (what, err)


def test_nonlinear_vjp_is_the_transpose_of_the_linearised_nonlinear_term():
    S, w, mean = setup(64, 64, TWO_PI, TWO_PI)
    kappa, dw = np.fft.rfft2(band_field(S, 2, 31)), np.fft.rfft2(band_field(S, 2, 32))
    e = 1e-5 * np.abs(w).max() / np.abs(dw).max()
    jvp = (S.nonlinear(w + e * dw, mean) - S.nonlinear(w - e * dw, mean)) / (2 * e)
    lhs, rhs = S.pair(kappa, jvp), S.pair(S.nonlinear_vjp(w, mean, kappa), dw)
    assert np.abs(lhs - rhs).max() <= 1e-8 * np.abs(lhs).max()


def test_init_and_velocity_adjoints():
    S, w, mean = setup(64, 128, 3.0, 7.0)
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal((2, 2, 64, 128))
    lam = np.fft.rfft2(band_field(S, 2, 41))
    ub, vb = S.init_vjp(lam)
    lhs, rhs = S.pair(S.init(u, v)[0], lam), (ub * u + vb * v).sum(axis=(-2, -1))
    assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(lhs).max()
    uu, vv = S.velocity(w, np.zeros_like(mean))
    lhs, rhs = (uu * u + vv * v).sum(axis=(-2, -1)), S.pair(S.velocity_vjp(u, v), w)
    assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(lhs).max()


def test_gradient_from_rest_is_the_decayed_projected_cotangent():
    S = A.AdjointScheme(64, 64, 0.01, 1.0, 1e-2, drag=0.3)
    rng = np.random.default_rng(9)
    mu = np.fft.rfft2(rng.standard_normal((1, 64, 64)))
    w = np.zeros_like(mu)
    wbar, gbar = S.step_vjp(w, np.zeros((1, 2)), mu, 3)
    ref = np.exp(-(S.nu * S.k2 + S.drag) * S.dt * 3) * S.M * mu
    assert np.abs(wbar - ref).max() <= 1e-13 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------- 2. wrong schemes on the GPU's inputs
@pytest.mark.parametrize('case', AC.CASES, ids=AC.case_id)
@pytest.mark.parametrize('wrong', A.WRONG)
def test_the_gpu_bound_would_catch_the_wrong_scheme(case, wrong):
    """Every wrong scheme sits >= 10x the GPU bound away from the right gradient, in wbar and (except where the mutation cannot reach it) in
    gbar.  The mean flow can only be missed where there is one: that mutation is checked on the case with a mean flow, and must be
    invisible on the others."""
    wbar, gbar = AC.oracle_gradient(case)
    wrong_w, wrong_g = AC.oracle_gradient(case, wrong)
    dw, dg = AC.rel(wrong_w, wbar), AC.rel(wrong_g, gbar)
    print('%s %s: wbar %.2e gbar %.2e' % (AC.case_id(case), wrong, dw, dg))
    if wrong == 'no_mean_flow' and case[5] == (0.0, 0.0):
        assert dw < 1e-9 and dg < 1e-9          # the grid mean of the float32 input is a rounding, not exactly zero
        return
    assert dw >= 10 * AC.BOUND and dg >= 10 * AC.BOUND, (dw, dg)


def test_bound_and_measurements():
    assert AC.BOUND < 1e-5
    assert set(AC.MEASURED) == set(AC.case_id(c) for c in AC.CASES)
    worst = max(max(v) for v in AC.MEASURED.values())
    assert 3 * worst <= AC.BOUND <= 7.5 * worst, (worst, AC.BOUND)
