"""CPU checks of the forward-mode restatement of the system with a scalar (tests/pspec_scalar_tangent_oracle.py) that the GPU step
(csrc/pspec_kernels.hip: nns_spec_ns_step_scalar_tangent_f32, through nns.periodic.PeriodicSolver.step_tangent_scalar) is compared against:
central differences of its own float64 forward, the dot-product identity against the reverse-mode restatement, the flow tangent's
restatement at b = 0, an eigenmode of the linear problem at rest, the distance of every deliberately wrong scheme from the right tangent on
the inputs of the GPU test, and the entry points."""
import inspect

import numpy as np
import pytest

import pspec_linear_cases as LC
import pspec_oracle as O
import pspec_scalar_tangent_cases as TC
import pspec_scalar_tangent_oracle as T
import pspec_tangent_oracle as FT

TWO_PI = 2 * np.pi
GRAD, BUOY = (0.7, -0.4), (0.6, 1.5)


def band_field(S, B, seed):
    return O.band_ic(B, S.nx, S.ny, seed, S.Lx, S.Ly, 1.0)[0]


def setup(nx, ny, Lx, Ly, linear, buoy=BUOY):
    """(S, w, t, mean, kw, force): a buoyant scheme with drag and a force, or with linear also hyperviscosity, hypofriction and beta."""
    B = 2
    u0, v0 = O.band_ic(B, nx, ny, 7 + nx + ny, Lx, Ly, 1.0, mean=(0.3, -0.2))
    dt = O.cfl_dt(nx, ny, Lx, Ly, 1.3)
    kw = dict(drag=0.2, kappa=2e-3, grad=GRAD, buoy=buoy, **(LC.params(nx, ny, Lx, Ly, dt) if linear else {}))
    S = T.ScalarTangentScheme(nx, ny, dt, 1.0, 1e-3, Lx, Ly, **kw)
    fx, fy = O.band_ic(B, nx, ny, 11, Lx, Ly, 0.5)
    S.set_forcing(fx, fy)
    w, mean = S.init(u0, v0)
    t = S.init_scalar(band_field(S, B, 13) + 0.25)
    return S, w, t, mean, kw, (fx, fy)


def directions(S):
    """(dw, dtheta, dg): directions of the state and of the source, dtheta with a mean."""
    dt = S.Mt * np.fft.rfft2(band_field(S, 2, 24) + 0.3)
    return S.M * np.fft.rfft2(band_field(S, 2, 22)), dt, S.M * np.fft.rfft2(band_field(S, 2, 23))


# ---------------------------------------------------------------------------------------------------- 1. central differences
@pytest.mark.parametrize('nx,ny,Lx,Ly', [(64, 64, TWO_PI, TWO_PI), (64, 128, 3.0, 7.0)])
@pytest.mark.parametrize('linear', [False, True], ids=['realE', 'complexE'])
@pytest.mark.parametrize('nsteps', [1, 3])
def test_step_jvp_against_central_differences(nx, ny, Lx, Ly, linear, nsteps):
    S, w, t, mean, _, _ = setup(nx, ny, Lx, Ly, linear)
    dw, dth, dg = directions(S)
    g0 = S.g

    def forward(ew, et, eg):
        S.g = g0 + eg * dg
        out = S.step(w + ew * dw, t + et * dth, mean, nsteps)
        S.g = g0
        return out

    zero = np.zeros_like(dw)
    scale = max(np.abs(w).max(), np.abs(t).max()) / max(np.abs(dw).max(), np.abs(dth).max())
    e = 1e-5 * scale
    for d, what in (((dw, zero, None), 'vorticity'), ((zero, dth, None), 'scalar'), ((dw, dth, None), 'state'), ((zero, zero, dg), 'source')):
        got = S.step_jvp(w, t, mean, d[0], d[1], nsteps, dg=d[2])
        on = [float(np.abs(x).max() > 0) if x is not None else 0.0 for x in d]
        # the source reaches theta^ only through du of later stages: a response of order dt^2, which the differences resolve with a 100x larger step
        h = 100 * e if what == 'source' else e
        hi, lo = forward(h * on[0], h * on[1], h * on[2]), forward(-h * on[0], -h * on[1], -h * on[2])
        errs = [TC.rel(got[i], (hi[i] - lo[i]) / (2 * h)) for i in (0, 1)]
        print('%s %dx%d %s nsteps=%d: jvp against central differences rel-L2 dw %.2e dtheta %.2e'
              % (what, nx, ny, 'complex E' if linear else 'real E', nsteps, errs[0], errs[1]))
        assert max(errs) <= 1e-7, (what, errs)


def test_nonlinear_jvp_against_central_differences():
    S, w, t, mean, _, _ = setup(64, 64, TWO_PI, TWO_PI, False)
    dw, dth, _ = directions(S)
    e = 1e-5 * np.abs(w).max() / np.abs(dw).max()
    nw, nt = S.nonlinear_jvp(w, t, mean, dw, dth)
    fw = (S.nonlinear_w(w + e * dw, t + e * dth, mean, 1) - S.nonlinear_w(w - e * dw, t - e * dth, mean, 1)) / (2 * e)
    ft = (S.nonlinear_scalar(w + e * dw, t + e * dth, mean) - S.nonlinear_scalar(w - e * dw, t - e * dth, mean)) / (2 * e)
    assert TC.rel(nw, fw) <= 1e-8 and TC.rel(nt, ft) <= 1e-8


# ---------------------------------------------------------------------------------------------------- 2. the dot-product identity
@pytest.mark.parametrize('linear', [False, True], ids=['realE', 'complexE'])
def test_step_jvp_is_the_transpose_of_step_vjp(linear):
    nx, ny, Lx, Ly, nsteps = 64, 128, 3.0, 7.0, 3
    S, w, t, mean, _, _ = setup(nx, ny, Lx, Ly, linear)
    dw, dth, dg = directions(S)
    rw, rt = np.fft.rfft2(band_field(S, 2, 21)), np.fft.rfft2(band_field(S, 2, 25) + 0.1)
    wbar, tbar, gbar = S.step_vjp(w, mean, rw, nsteps, t=t, mu=rt)
    jw, jt = S.step_jvp(w, t, mean, dw, dth, nsteps, dg=dg)
    lhs = S.pair(jw, rw) + S.pair(jt, rt)
    rhs = S.pair(wbar, dw) + S.pair(tbar, dth) + S.pair(gbar, dg)
    err = np.abs(lhs - rhs).max() / np.abs(lhs).max()
    print('<J d, r> = <d, J^T r> rel %.2e' % err)
    assert err <= 1e-12, err


# ---------------------------------------------------------------------------------------------------- 3. exact cases
@pytest.mark.parametrize('linear', [False, True], ids=['realE', 'complexE'])
def test_without_buoyancy_the_vorticity_half_is_the_flow_tangent(linear):
    nx, ny, Lx, Ly = 64, 64, TWO_PI, TWO_PI
    S, w, t, mean, kw, (fx, fy) = setup(nx, ny, Lx, Ly, linear, buoy=(0.0, 0.0))
    F = FT.TangentScheme(nx, ny, S.dt, 1.0, 1e-3, Lx, Ly, **{k: v for k, v in kw.items() if k not in ('kappa', 'grad', 'buoy')})
    F.set_forcing(fx, fy)
    dw, dth, dg = directions(S)
    got = S.step_jvp(w, t, mean, dw, dth, 3, dg=dg)[0]
    assert np.array_equal(got, F.step_jvp(w, mean, dw, 3, dg=dg))


def test_the_mean_of_dtheta_is_carried_unchanged():
    S, w, t, mean, _, _ = setup(64, 64, TWO_PI, TWO_PI, False)
    dw, dth, dg = directions(S)
    out = S.step_jvp(w, t, mean, dw, dth, 3, dg=dg)[1]
    assert np.abs(out[:, 0, 0] - dth[:, 0, 0]).max() <= 1e-12 * np.abs(dth[:, 0, 0]).max()


def test_an_eigenmode_from_rest_grows_at_its_rate():
    p = TC.EIGEN
    S = T.ScalarTangentScheme(p['nx'], p['ny'], p['dt'], 1.0, p['nu'], drag=p['drag'], kappa=p['kappa'], grad=p['G'], buoy=p['b'])
    dw0, dt0, lam = TC.eigenmode(0.0)[:3]
    assert abs(lam - TC.EIGEN_EXPONENT) <= 1e-9
    zero = np.zeros((1, p['nx'], p['ny'] // 2 + 1), dtype=np.complex128)
    n = p['nsteps']
    dw, dth = S.step_jvp(zero, zero, np.array([p['U']]), np.fft.rfft2(dw0[None]), np.fft.rfft2(dt0[None]), n)
    rw, rt, _, aw, at = TC.eigenmode(n * p['dt'])
    ew, et = np.abs(S.irfft2(dw)[0] - rw).max() / aw, np.abs(S.irfft2(dth)[0] - rt).max() / at
    rate = np.log(np.linalg.norm(dw) / np.linalg.norm(np.fft.rfft2(dw0))) / (n * p['dt'])
    print('eigenmode %s: exponent %.9f; after %d steps max error / amplitude dw %.2e dtheta %.2e, growth rate %.9f (error %.2e)'
          % (p['m'], lam, n, ew, et, rate, abs(rate - lam)))
    assert max(ew, et) <= 1e-8 and abs(rate - lam) <= 1e-8


# ---------------------------------------------------------------------------------------------------- 4. wrong schemes on the GPU's inputs
def invisible(kind, wrong):
    """The wrong scheme cannot show in this kind's run: the buoyancy's mistakes without buoyancy."""
    return wrong in ('no_dbuoy', 'buoy_sign') and TC.KINDS[kind][0] == (0.0, 0.0)


# The one pair without the factor of 10: theta frozen at the step's start under the PASSIVE scalar at 1024 x 64.  Without buoyancy the mistake
# acts only through du . (grad theta_i - grad theta_0) in dN_theta, and on that case's inputs theta moves so little within a step that the
# wrong scheme lies 1.13e-6 from the right one in dtheta^ (exactly 0 in dw^) -- the size of the bound, not 10x it.  Neither remedy changes
# that: more steps leave it where it is (1.13e-6, 1.31e-6, 1.20e-6 after 3, 6, 12 steps: the error made per step does not accumulate
# relative to the tangent), and a passive run has no buoyancy to raise.  The same mistake is caught with the factor of 10 at every other
# run (>= 2.4e-5 in dtheta^; in the buoyant run of this shape by 1.05e-5 in dw^), so the pair is recorded here with its figure, not hidden.
FAINT = ('frozen_theta', 'passive-1024x64x2')


@pytest.mark.parametrize('run', TC.RUNS, ids=TC.run_id)
@pytest.mark.parametrize('wrong', T.WRONG)
def test_the_gpu_bounds_would_catch_the_wrong_scheme(run, wrong):
    """Every wrong scheme sits >= 10x the GPU bound away from the right tangent in dw^ or in dtheta^ (with the per-grid source perturbation),
    where it can show; a mistake in the buoyancy is invisible without one."""
    kind, case = run
    right, bad = TC.oracle_tangent(run, None, 'grid'), TC.oracle_tangent(run, wrong, 'grid')
    dw, dt = TC.rel(bad[0], right[0]), TC.rel(bad[1], right[1])
    print('%s %s: dw %.2e dtheta %.2e' % (TC.run_id(run), wrong, dw, dt))
    if invisible(kind, wrong):
        assert max(dw, dt) < 1e-9, (dw, dt)
        return
    if (wrong, TC.run_id(run)) == FAINT:
        assert TC.BOUND_T <= dt <= 2e-6 and dw == 0.0, (dw, dt)
        return
    assert dw >= 10 * TC.BOUND_W or dt >= 10 * TC.BOUND_T, (dw, dt)


def test_the_mean_gradient_is_invisible_where_there_is_none():
    run = ('buoyant', TC.CASES[0])
    right, bad = (TC.oracle_tangent(run, wrong, None, grad=(0.0, 0.0)) for wrong in (None, 'no_G'))
    assert max(TC.rel(bad[0], right[0]), TC.rel(bad[1], right[1])) < 1e-9


def test_bound_and_measurements():
    assert TC.BOUND_W < 1e-5 and TC.BOUND_T < 1e-5
    assert set(TC.MEASURED) == set(TC.run_id(r) for r in TC.RUNS)
    for i, bound in ((0, TC.BOUND_W), (1, TC.BOUND_T)):
        worst = max(v[i] for v in TC.MEASURED.values())
        assert 3 * worst <= bound <= 7 * worst, (worst, bound)
    assert set(TC.DOT_MEASURED) == set(TC.DOT_KINDS)
    worst = max(TC.DOT_MEASURED.values())
    assert 3 * worst <= TC.DOT_BOUND <= 7 * worst, (worst, TC.DOT_BOUND)


# ---------------------------------------------------------------------------------------------------- 5. the entry points
def test_the_solver_and_the_binding_have_the_scalar_forward_mode():
    from nns import _lib, ops
    from nns.periodic import PeriodicSolver
    names = _lib.exported_names()
    assert 'nns_spec_ns_step_scalar_tangent_f32' in names and 'nns_spec_ns_scalar_tangent_workspace' in names
    assert callable(ops.spec_ns_scalar_tangent_workspace) and callable(ops.spec_ns_step_scalar_tangent_)
    par = lambda f: list(inspect.signature(f).parameters)
    assert par(PeriodicSolver.step_tangent_scalar) == ['self', 'state', 'dwhat', 'dthat', 'nsteps', 'dforcing']
    assert par(PeriodicSolver.evolve_tangent_scalar) == ['self', 'w', 'theta', 'dw', 'dtheta', 'nsteps', 'mean', 'forcing', 'dforcing', 'clock',
                                                         'noise_ids']
    assert par(PeriodicSolver.evolve_velocity_tangent_scalar) == ['self', 'u0', 'v0', 'theta0', 'du0', 'dv0', 'dtheta0', 'nsteps', 'forcing',
                                                                  'dforcing', 'clock', 'noise_ids']
    assert par(PeriodicSolver.lyapunov_exponent_scalar) == ['self', 'state', 'dwhat', 'dthat', 'nsteps', 'renormalize_every', 'scalar_weight']
    assert inspect.signature(PeriodicSolver.lyapunov_exponent_scalar).parameters['scalar_weight'].default == 1.0
