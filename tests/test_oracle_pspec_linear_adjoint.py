"""CPU checks of the reverse-mode restatement (tests/pspec_linear_adjoint_oracle.py) that the GPU adjoint of the periodic solver's linear step
(csrc/pspec_kernels.hip: nns_spec_ns_step_linear_adjoint_f32, through nns.periodic.PeriodicSolver.evolve) is compared against: the dot-product
identity against central differences of its own forward (LinearScheme.step, and the stochastic run with its noise held fixed), its agreement
with the two parent restatements when the three linear terms are zero, and the distance of every deliberately wrong scheme from the right
gradient on the inputs of the GPU test.  One test needs the package and its binding, not the GPU: the entry points exist."""
import numpy as np
import pytest

import pspec_linear_adjoint_cases as LA
import pspec_linear_adjoint_oracle as A
import pspec_linear_cases as LC
import pspec_oracle as O
import pspec_stochastic_oracle as ST

TWO_PI = 2 * np.pi


def band_field(S, B, seed):
    """A real field whose spectrum fills the kept band (zero mean)."""
    return O.band_ic(B, S.nx, S.ny, seed, S.Lx, S.Ly, 1.0)[0]


def setup(nx, ny, Lx, Ly, scalar, linear=True):
    """(S, w, t or None, mean): every term acting (the parameters of pspec_linear_cases at this shape), a per-grid force, a mean flow."""
    B = 2
    u0, v0 = O.band_ic(B, nx, ny, 7 + nx + ny, Lx, Ly, 1.0, mean=(0.3, -0.2))
    dt = O.cfl_dt(nx, ny, Lx, Ly, 1.3)
    kw = LC.params(nx, ny, Lx, Ly, dt) if linear else {}
    if scalar:
        kw.update(kappa=2e-3, grad=(0.7, -0.4), buoy=(0.6, 1.5))
    S = A.LinearAdjointScheme(nx, ny, dt, 1.0, 1e-3, Lx, Ly, drag=0.2, **kw)
    fx, fy = O.band_ic(B, nx, ny, 11, Lx, Ly, 0.5)
    S.set_forcing(fx, fy)
    w, mean = S.init(u0, v0)
    return S, w, (S.init_scalar(band_field(S, B, 12) + 0.25) if scalar else None), mean


def identity(S, w, t, mean, nsteps, forward, vjp, tag):
    """The dot-product identity of vjp against central differences of forward(w, t) -> (w, t), in w, theta and g; returns the worst error."""
    scalar = t is not None
    lam, mu = np.fft.rfft2(band_field(S, 2, 21)), np.fft.rfft2(band_field(S, 2, 24) + 0.1)
    dw, dth, dg = np.fft.rfft2(band_field(S, 2, 22)), np.fft.rfft2(band_field(S, 2, 25) + 0.3), np.fft.rfft2(band_field(S, 2, 23))
    out = vjp(lam, mu)
    wbar, tbar, gbar = out if scalar else (out[0], None, out[1])
    g0 = S.g

    def loss(eps_w, eps_t, eps_g):
        S.g = g0 + eps_g * dg
        ow, ot = forward(w + eps_w * dw, t + eps_t * dth if scalar else None)
        S.g = g0
        return S.pair(ow, lam) + (S.pair(ot, mu) if scalar else 0.0)

    central = lambda k: (lambda e: (loss(*(e * np.eye(3)[k])) - loss(*(-e * np.eye(3)[k]))) / (2 * e))
    # the source acts through dt g per step: its step is 1 / (nsteps dt) larger (tests/test_oracle_pspec_scalar_adjoint.py)
    checks = [(S.pair(wbar, dw), central(0), np.abs(w).max() / np.abs(dw).max(), 'w'),
              (S.pair(gbar, dg), central(2), np.abs(w).max() / np.abs(dg).max() / (nsteps * S.dt), 'g')]
    if scalar:
        checks.append((S.pair(tbar, dth), central(1), np.abs(t).max() / np.abs(dth).max(), 'theta'))
    worst = 0.0
    for got, fd, scale, what in checks:
        ref = fd(1e-6 * scale)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print('%s %s %dx%d nsteps=%d: dot-product identity rel %.2e' % (tag, what, S.nx, S.ny, nsteps, err))
        worst = max(worst, err)
    return worst


# ---------------------------------------------------------------------------------------------------- 1. the dot-product identity
# the precision the two sibling files reach on their own forwards (measured <= 4e-9 and <= 1e-9; they assert 1e-7 and 1e-8)
FD_BOUND = 1e-8


@pytest.mark.parametrize('nx,ny,Lx,Ly', [(64, 64, TWO_PI, TWO_PI), (64, 128, 3.0, 7.0)])
@pytest.mark.parametrize('nsteps', [1, 3])
@pytest.mark.parametrize('scalar', [False, True], ids=['flow', 'scalar'])
def test_step_vjp_against_central_differences(nx, ny, Lx, Ly, nsteps, scalar):
    S, w, t, mean = setup(nx, ny, Lx, Ly, scalar)
    assert np.abs(S.factors()[0].imag).max() > 0.05                       # the factors are complex here
    if scalar:
        forward = lambda w_, t_: S.step(w_, t_, mean, nsteps)
        vjp = lambda lam, mu: S.step_vjp(w, mean, lam, nsteps, t=t, mu=mu)
    else:
        forward = lambda w_, t_: (S.step(w_, mean, nsteps), None)
        vjp = lambda lam, mu: S.step_vjp(w, mean, lam, nsteps)
    assert identity(S, w, t, mean, nsteps, forward, vjp, 'linear') <= FD_BOUND


@pytest.mark.parametrize('scalar', [False, True], ids=['flow', 'scalar'])
def test_stochastic_vjp_against_central_differences_with_the_noise_held_fixed(scalar):
    """The kicks are the same numbers on both sides of the difference: they drop out of the quotient, and what remains is the deterministic
    step's Jacobian about the noisy trajectory."""
    nx, ny, nsteps = 64, 64, 3
    S, w, t, mean = setup(nx, ny, TWO_PI, TWO_PI, scalar)
    rate = float(np.mean(S.diag(w)[0]) / (nsteps * S.dt))                 # kicks of the state's size
    amp = ST.amplitude_table(nx, ny, TWO_PI, TWO_PI, ST.ring_rates(nx, ny, TWO_PI, TWO_PI, rate, 4.0, 6.0))
    X = ST.Stochastic(S, amp, 5)
    if scalar:
        forward = lambda w_, t_: X.step(w_, mean, nsteps, t=t_, n0=7)
    else:
        forward = lambda w_, t_: (X.step(w_, mean, nsteps, n0=7), None)
    end = forward(w, t)[0]
    assert LA.rel(end, S.step(w, t, mean, nsteps)[0] if scalar else S.step(w, mean, nsteps)) > 0.05       # the noise is no perturbation
    vjp = lambda lam, mu: A.stochastic_vjp(S, amp, 5, w, mean, lam, nsteps, t=t, mu=mu if scalar else None, n0=7)
    assert identity(S, w, t, mean, nsteps, forward, vjp, 'stochastic') <= FD_BOUND
    # about the kick-free trajectory the identity fails by far more than the differences' own error
    wrong = lambda lam, mu: A.stochastic_vjp(S, amp, 5, w, mean, lam, nsteps, t=t, mu=mu if scalar else None, n0=7, wrong='kicks_dropped')
    assert identity(S, w, t, mean, nsteps, forward, wrong, 'kicks_dropped') > 1e3 * FD_BOUND


# ---------------------------------------------------------------------------------------------------- 2. no linear terms: the parents
def test_without_the_linear_terms_the_restatement_is_the_parents():
    import pspec_adjoint_oracle as PA
    import pspec_scalar_adjoint_oracle as SA
    S, w, t, mean = setup(64, 64, TWO_PI, TWO_PI, False, linear=False)
    lam, mu = np.fft.rfft2(band_field(S, 2, 21)), np.fft.rfft2(band_field(S, 2, 24) + 0.1)
    P = PA.AdjointScheme(64, 64, S.dt, 1.0, S.nu, drag=S.drag)
    P.g = S.g
    for got, ref in zip(S.step_vjp(w, mean, lam, 2), P.step_vjp(w, mean, lam, 2)):
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    S, w, t, mean = setup(64, 64, TWO_PI, TWO_PI, True, linear=False)
    P = SA.ScalarAdjointScheme(64, 64, S.dt, 1.0, S.nu, drag=S.drag, kappa=S.kappa, grad=S.grad, buoy=S.buoy)
    P.g = S.g
    for got, ref in zip(S.step_vjp(w, mean, lam, 2, t=t, mu=mu), P.step_vjp(w, t, mean, lam, mu, 2)):
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_a_wave_at_rest_turns_backwards_in_the_cotangent():
    """No flow, no force: the step is w -> E^2 w, so wbar = conj(E^2)^n M lam exactly -- the rotation of the Rossby wave undone."""
    S = A.LinearAdjointScheme(64, 64, 0.05, 1.0, 1e-2, drag=0.3, hyper=(1e-9, 4), hypo=(0.02, 1), beta=4.0)
    lam = np.fft.rfft2(np.random.default_rng(3).standard_normal((1, 64, 64)))
    z = np.zeros_like(lam)
    wbar, gbar = S.step_vjp(z, np.zeros((1, 2)), lam, 3)
    ref = np.conj(S.factors()[1]) ** 3 * S.M * lam
    assert np.abs(np.angle(S.factors()[1])).max() > 0.1                  # radians per step on the gravest x-mode: it does turn
    assert np.abs(wbar - ref).max() <= 1e-13 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------- 3. wrong schemes on the GPU's inputs
WRONG_RUNS = [(run, w) for run in LA.RUNS for w in A.WRONG + (A.WRONG_STOCHASTIC if run[0] == 'stochastic' else ())]


@pytest.mark.parametrize('run,wrong', WRONG_RUNS, ids=['%s-%s' % (LA.run_id(r), w) for r, w in WRONG_RUNS])
def test_the_gpu_bound_would_catch_the_wrong_scheme(run, wrong):
    """Every wrong scheme sits >= 10x the GPU bound away from the right gradient in the worst of wbar, (thetabar,) gbar."""
    kind, case = run
    right, got = LA.oracle_gradient(kind, case), LA.oracle_gradient(kind, case, wrong)
    d = [LA.rel(g, r) for g, r in zip(got, right)]
    print('%s %s: %s' % (LA.run_id(run), wrong, ' '.join('%.2e' % x for x in d)))
    assert max(d) >= 10 * LA.bound(kind), d


def test_bounds_and_measurements():
    """The bounds are the parents' (the measured errors stay under them), under the README's target; one measurement per run."""
    import pspec_adjoint_cases as AC
    import pspec_scalar_adjoint_cases as SAC
    assert LA.BOUND_FLOW == AC.BOUND == 4e-6 and LA.BOUND_SCALAR == SAC.BOUND == 3e-6 and max(LA.BOUND_FLOW, LA.BOUND_SCALAR) < 1e-5
    assert set(LA.MEASURED) == set(LA.run_id(r) for r in LA.RUNS)
    for run in LA.RUNS:
        assert max(LA.MEASURED[LA.run_id(run)]) < LA.bound(run[0]), run


# ---------------------------------------------------------------------------------------------------- 4. the entry points exist
def test_the_solver_and_the_binding_have_the_linear_adjoint():
    from nns import _lib
    from nns.periodic import PeriodicSolver
    assert callable(getattr(PeriodicSolver, 'evolve')) and callable(getattr(PeriodicSolver, 'evolve_velocity'))
    assert 'nns_spec_ns_step_linear_adjoint_f32' in set(_lib.exported_names())
    assert _lib.lib().nns_spec_ns_step_linear_adjoint_f32 is not None
