"""CPU checks of the forward-mode restatement (tests/pspec_tangent_oracle.py) that the GPU tangent-linear step of the periodic solver
(csrc/pspec_kernels.hip: nns_spec_ns_step_tangent_f32, through nns.periodic.PeriodicSolver.step_tangent) is compared against: central
differences of its own float64 forward, the dot-product identity against the reverse-mode restatements, the distance of every deliberately
wrong scheme from the right tangent on the inputs of the GPU test, and the entry points."""
import inspect

import numpy as np
import pytest

import pspec_adjoint_oracle as A
import pspec_linear_adjoint_oracle as LA
import pspec_linear_cases as LC
import pspec_oracle as O
import pspec_tangent_cases as TC
import pspec_tangent_oracle as T

TWO_PI = 2 * np.pi


def band_field(S, B, seed):
    return O.band_ic(B, S.nx, S.ny, seed, S.Lx, S.Ly, 1.0)[0]


def setup(nx, ny, Lx, Ly, linear):
    """(S, w, mean, kw): a forced scheme with drag, or with linear also hyperviscosity, hypofriction and beta (complex E); kw its arguments."""
    B = 2
    u0, v0 = O.band_ic(B, nx, ny, 7 + nx + ny, Lx, Ly, 1.0, mean=(0.3, -0.2))
    dt = O.cfl_dt(nx, ny, Lx, Ly, 1.3)
    kw = dict(drag=0.2, **(LC.params(nx, ny, Lx, Ly, dt) if linear else {}))
    S = T.TangentScheme(nx, ny, dt, 1.0, 1e-3, Lx, Ly, **kw)
    fx, fy = O.band_ic(B, nx, ny, 11, Lx, Ly, 0.5)
    S.set_forcing(fx, fy)
    w, mean = S.init(u0, v0)
    return S, w, mean, kw, (fx, fy)


# ---------------------------------------------------------------------------------------------------- 1. central differences
@pytest.mark.parametrize('nx,ny,Lx,Ly', [(64, 64, TWO_PI, TWO_PI), (64, 128, 3.0, 7.0)])
@pytest.mark.parametrize('linear', [False, True], ids=['realE', 'complexE'])
@pytest.mark.parametrize('nsteps', [1, 3])
def test_step_jvp_against_central_differences(nx, ny, Lx, Ly, linear, nsteps):
    S, w, mean, _, _ = setup(nx, ny, Lx, Ly, linear)
    dw = S.M * np.fft.rfft2(band_field(S, 2, 22))              # a direction of the state
    dg = S.M * np.fft.rfft2(band_field(S, 2, 23))              # a direction of the source
    g0 = S.g

    def forward(eps_w, eps_g):
        S.g = g0 + eps_g * dg
        out = S.step(w + eps_w * dw, mean, nsteps)
        S.g = g0
        return out

    e = 1e-5 * np.abs(w).max() / np.abs(dw).max()
    zero = np.zeros_like(dw)
    for got, fd, what in ((S.step_jvp(w, mean, dw, nsteps), (forward(e, 0.0) - forward(-e, 0.0)) / (2 * e), 'state'),
                          (S.step_jvp(w, mean, zero, nsteps, dg=dg), (forward(0.0, e) - forward(0.0, -e)) / (2 * e), 'source')):
        err = TC.rel(got, fd)
        print('%s %dx%d %s nsteps=%d: jvp against central differences rel-L2 %.2e' % (what, nx, ny, 'complex E' if linear else 'real E', nsteps, err))
        assert err <= 1e-7, (what, err)


def test_nonlinear_jvp_against_central_differences():
    S, w, mean, _, _ = setup(64, 64, TWO_PI, TWO_PI, False)
    dw = S.M * np.fft.rfft2(band_field(S, 2, 32))
    e = 1e-5 * np.abs(w).max() / np.abs(dw).max()
    fd = (S.nonlinear(w + e * dw, mean) - S.nonlinear(w - e * dw, mean)) / (2 * e)
    assert TC.rel(S.nonlinear_jvp(w, mean, dw), fd) <= 1e-8


# ---------------------------------------------------------------------------------------------------- 2. the dot-product identity
@pytest.mark.parametrize('linear', [False, True], ids=['AdjointScheme', 'LinearAdjointScheme'])
def test_step_jvp_is_the_transpose_of_the_reverse_mode_restatement(linear):
    nx, ny, Lx, Ly, nsteps = 64, 128, 3.0, 7.0, 3
    S, w, mean, kw, (fx, fy) = setup(nx, ny, Lx, Ly, linear)
    R = LA.LinearAdjointScheme(nx, ny, S.dt, 1.0, 1e-3, Lx, Ly, **kw) if linear else A.AdjointScheme(nx, ny, S.dt, 1.0, 1e-3, Lx, Ly, **kw)
    R.set_forcing(fx, fy)
    dw, dg, r = (np.fft.rfft2(band_field(S, 2, s)) for s in (22, 23, 21))
    wbar, gbar = R.step_vjp(w, mean, r, nsteps)
    lhs = S.pair(S.step_jvp(w, mean, dw, nsteps, dg=dg), r)
    rhs = S.pair(wbar, dw) + S.pair(gbar, dg)
    err = np.abs(lhs - rhs).max() / np.abs(lhs).max()
    print('<J d, r> = <d, J^T r> rel %.2e' % err)
    assert err <= 1e-12, err


def test_tangent_from_rest_is_the_translated_damped_perturbation():
    S = T.TangentScheme(64, 64, 0.01, 1.0, 1e-2, drag=0.3)
    dw = S.M * np.fft.rfft2(np.random.default_rng(9).standard_normal((1, 64, 64)))
    out = S.step_jvp(np.zeros_like(dw), np.zeros((1, 2)), dw, 3)
    ref = np.exp(-(S.nu * S.k2 + S.drag) * S.dt * 3) * dw
    assert np.abs(out - ref).max() <= 1e-13 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------- 3. wrong schemes on the GPU's inputs
@pytest.mark.parametrize('run', TC.RUNS, ids=TC.run_id)
@pytest.mark.parametrize('wrong', T.WRONG)
def test_the_gpu_bound_would_catch_the_wrong_scheme(run, wrong):
    """Every wrong scheme sits >= 10x the GPU bound away from the right tangent (with the per-grid source perturbation, so that a source
    mutation shows).  The mean flow can only be missed where there is one, and conj(E) differs from E only in the linear form: those are
    checked where they can show and must be invisible elsewhere."""
    kind, case = run
    right, bad = TC.oracle_tangent(run, None, 'grid'), TC.oracle_tangent(run, wrong, 'grid')
    d = TC.rel(bad, right)
    print('%s %s: %.2e' % (TC.run_id(run), wrong, d))
    if (wrong == 'no_mean_flow' and case[5] == (0.0, 0.0)) or (wrong == 'conj_E' and kind != 'linear'):
        assert d < 1e-9, d                      # the grid mean of the float32 input is a rounding, not exactly zero
        return
    assert d >= 10 * TC.BOUND, d


def test_bound_and_measurements():
    assert TC.BOUND < 1e-5
    assert set(TC.MEASURED) == set(TC.run_id(r) for r in TC.RUNS)
    worst = max(max(v) for v in TC.MEASURED.values())
    assert 3 * worst <= TC.BOUND <= 7 * worst, (worst, TC.BOUND)
    assert set(TC.DOT_MEASURED) == set(TC.KINDS)
    worst = max(TC.DOT_MEASURED.values())
    assert 3 * worst <= TC.DOT_BOUND <= 7 * worst, (worst, TC.DOT_BOUND)


# ---------------------------------------------------------------------------------------------------- 4. the entry points
def test_the_solver_and_the_binding_have_the_forward_mode():
    from nns import _lib, ops
    from nns.periodic import PeriodicSolver
    names = _lib.exported_names()
    assert 'nns_spec_ns_step_tangent_f32' in names and 'nns_spec_ns_tangent_workspace' in names
    assert callable(ops.spec_ns_tangent_workspace) and callable(ops.spec_ns_step_tangent_)
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(PeriodicSolver.step_tangent) == ['self', 'state', 'dwhat', 'nsteps', 'dforcing']
    assert par(PeriodicSolver.evolve_tangent) == ['self', 'w', 'dw', 'nsteps', 'mean', 'forcing', 'dforcing', 'clock', 'noise_ids']
    assert par(PeriodicSolver.evolve_velocity_tangent) == ['self', 'u0', 'v0', 'du0', 'dv0', 'nsteps', 'forcing', 'dforcing', 'clock', 'noise_ids']
    assert par(PeriodicSolver.lyapunov_exponent) == ['self', 'state', 'dwhat', 'nsteps', 'renormalize_every']
