"""CPU checks of the restatement (tests/pspec_operator_grad_oracle.py) that the GPU gradient of the periodic solver in its linear operator
(csrc/pspec_kernels.hip: nns_spec_ns_step_operator_adjoint_f32, through nns.periodic.PeriodicSolver.evolve with ``operator``) is compared
against: central differences of its own forward in random admissible perturbations of the table and in each of nu, drag, nu_h, mu, beta
through the table's formula, the defining properties of the result, and the distance of every deliberately wrong gradient from the right
one on the inputs of the GPU test.  One test needs the package and its binding, not the GPU: the entry points exist."""
import numpy as np
import pytest

import pspec_linear_adjoint_cases as LA
import pspec_linear_cases as LC
import pspec_operator_grad_cases as OC
import pspec_operator_grad_oracle as G
import pspec_oracle as O
import pspec_stochastic_oracle as ST
from test_oracle_pspec_linear_adjoint import FD_BOUND, band_field

TWO_PI = 2 * np.pi


def setup(nx, ny, Lx, Ly, scalar, **over):
    """(S, w, t or None, mean): test_oracle_pspec_linear_adjoint.setup on an OperatorGradScheme -- every term acting, a per-grid force, a mean
    flow; ``over`` replaces parameters (the central differences in them)."""
    B = 2
    u0, v0 = O.band_ic(B, nx, ny, 7 + nx + ny, Lx, Ly, 1.0, mean=(0.3, -0.2))
    dt = O.cfl_dt(nx, ny, Lx, Ly, 1.3)
    kw = dict(LC.params(nx, ny, Lx, Ly, dt), nu=1e-3, drag=0.2)
    if scalar:
        kw.update(kappa=2e-3, grad=(0.7, -0.4), buoy=(0.6, 1.5))
    kw.update(over)
    nu = kw.pop('nu')
    S = G.OperatorGradScheme(nx, ny, dt, 1.0, nu, Lx, Ly, **kw)
    fx, fy = O.band_ic(B, nx, ny, 11, Lx, Ly, 0.5)
    S.set_forcing(fx, fy)
    w, mean = S.init(u0, v0)
    return S, w, (S.init_scalar(band_field(S, B, 12) + 0.25) if scalar else None), mean


def cotangents(S):
    return np.fft.rfft2(band_field(S, 2, 21)), np.fft.rfft2(band_field(S, 2, 24) + 0.1)


def loss(S, w, t, mean, nsteps, lam, mu, forward=None):
    """L per grid = <w(nsteps), lam> (+ <theta(nsteps), mu>) of the scheme as it stands (its table, or its parameters)."""
    if forward is not None:
        ow, ot = forward(w, t)
    elif t is None:
        ow, ot = S.step(w, mean, nsteps), None
    else:
        ow, ot = S.step(w, t, mean, nsteps)
    return S.pair(ow, lam) + (S.pair(ot, mu) if t is not None else 0.0)


def worst(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------- 1. central differences in the table
@pytest.mark.parametrize('nx,ny,Lx,Ly', [(64, 64, TWO_PI, TWO_PI), (64, 128, 3.0, 7.0)])
@pytest.mark.parametrize('nsteps', [1, 3])
@pytest.mark.parametrize('scalar', [False, True], ids=['flow', 'scalar'])
def test_table_gradient_against_central_differences(nx, ny, Lx, Ly, nsteps, scalar):
    """Random admissible perturbations dl (l(-k) = conj(l(k)) on the ky = 0 line) of the parameters' own table, real and imaginary parts at
    once and one at a time: sum over the stored entries of G . dl against (L(l + e dl) - L(l - e dl)) / 2 e.  The bound is the one
    test_oracle_pspec_linear_adjoint.py holds its own central differences to."""
    S, w, t, mean = setup(nx, ny, Lx, Ly, scalar)
    lam, mu = cotangents(S)
    Gt = S.operator_vjp(w, mean, lam, nsteps, t=t, mu=mu if scalar else None)[None]
    base = S.parameter_table()
    assert np.abs(base.imag).max() > 0.05 and base.real.min() < -2.0                   # complex factors, a stiff corner
    rng = np.random.default_rng(5)
    for part in ('both', 'real', 'imag'):
        dl = S.M * G.symmetric_table(rng, S)
        dl = dl if part == 'both' else dl.real + 0j if part == 'real' else 1j * dl.imag
        e = 1e-6 / np.abs(dl).max()
        L = []
        for sign in (1.0, -1.0):
            S.table = base + sign * e * dl
            L.append(loss(S, w, t, mean, nsteps, lam, mu))
        S.table = None
        ref = (L[0] - L[1]) / (2 * e)
        got = S.stored_pairing(Gt, dl)
        err = worst(got, ref)
        print('table %s %dx%d nsteps=%d %s: rel %.2e' % ('scalar' if scalar else 'flow', nx, ny, nsteps, part, err))
        assert err <= FD_BOUND


def test_a_table_is_the_parameters_scheme():
    """With table = parameter_table() the scheme steps as the parent does from its parameters (so the differences above are about the solver's
    own operator), and the parent's cotangents are untouched."""
    S, w, t, mean = setup(64, 64, TWO_PI, TWO_PI, True)
    ref = S.step(w, t, mean, 2)
    S.table = S.parameter_table()
    got = S.step(w, t, mean, 2)
    for a, b in zip(got, ref):
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


# ---------------------------------------------------------------------------------------------------- 2. central differences in the parameters
@pytest.mark.parametrize('name', OC.PARAMETERS)
@pytest.mark.parametrize('scalar', [False, True], ids=['flow', 'scalar'])
def test_parameter_gradient_against_central_differences(name, scalar):
    """d L / d nu, drag, nu_h, mu, beta: the table gradient paired with the formula's partial derivative, against central differences of the
    scheme rebuilt with the parameter moved.  The fourth-order stencil with a relative step of 1e-3: the two-point quotient that the table's
    test uses cannot reach the bound here, because the loss is large against its sensitivity to one number (with a relative step of 1e-5
    the rounding of L alone is 1.4e-8 of d L / d nu, and a larger step brings the quotient's own h^2 term up); the stencil's h^4 term is
    ~1e-12 and the rounding ~1e-10."""
    nx, ny, nsteps = 64, 64, 3
    S, w, t, mean = setup(nx, ny, TWO_PI, TWO_PI, scalar)
    lam, mu = cotangents(S)
    Gt = S.operator_vjp(w, mean, lam, nsteps, t=t, mu=mu if scalar else None)[None]
    got = S.stored_pairing(Gt, S.parameter_derivatives()[name])
    value = dict(nu=S.nu, drag=S.drag, nu_h=S.hyper[0], mu=S.hypo[0], beta=S.beta)[name]
    assert value != 0.0
    e = 1e-3 * abs(value)
    L = {}
    for m in (-2, -1, 1, 2):
        x = value + m * e
        over = {'nu_h': dict(hyper=(x, S.hyper[1])), 'mu': dict(hypo=(x, S.hypo[1]))}.get(name, {name: x})
        P, w_, t_, mean_ = setup(nx, ny, TWO_PI, TWO_PI, scalar, **over)
        L[m] = loss(P, w_, t_, mean_, nsteps, lam, mu)
    ref = (8 * (L[1] - L[-1]) - (L[2] - L[-2])) / (12 * e)
    err = worst(got, ref)
    print('parameter %s (%s): %s against %s, rel %.2e' % (name, 'scalar' if scalar else 'flow', got, ref, err))
    assert err <= FD_BOUND


def test_stochastic_table_gradient_with_the_noise_held_fixed():
    """The kicks do not depend on the table: they are the same numbers on both sides of the difference."""
    nx, ny, nsteps = 64, 64, 3
    S, w, t, mean = setup(nx, ny, TWO_PI, TWO_PI, False)
    rate = float(np.mean(S.diag(w)[0]) / (nsteps * S.dt))                 # kicks of the state's size
    amp = ST.amplitude_table(nx, ny, TWO_PI, TWO_PI, ST.ring_rates(nx, ny, TWO_PI, TWO_PI, rate, 4.0, 6.0))
    X = ST.Stochastic(S, amp, 5)
    forward = lambda w_, t_: (X.step(w_, mean, nsteps, n0=7), None)
    lam, mu = cotangents(S)
    Gt = G.stochastic_operator_vjp(S, amp, 5, w, mean, lam, nsteps, n0=7)[None]
    quiet = S.operator_vjp(w, mean, lam, nsteps)[None]
    assert LA.rel(Gt, quiet) > 0.05                                       # the noise is no perturbation
    base = S.parameter_table()
    dl = S.M * G.symmetric_table(np.random.default_rng(6), S)
    e = 1e-6 / np.abs(dl).max()
    L = []
    for sign in (1.0, -1.0):
        S.table = base + sign * e * dl
        L.append(loss(S, w, None, mean, nsteps, lam, mu, forward))
    S.table = None
    err = worst(S.stored_pairing(Gt, dl), (L[0] - L[1]) / (2 * e))
    print('stochastic table: rel %.2e' % err)
    assert err <= FD_BOUND


# ---------------------------------------------------------------------------------------------------- 3. the defining properties
def test_the_gradient_is_symmetric_on_the_line_and_zero_off_the_band():
    S, w, t, mean = setup(64, 64, TWO_PI, TWO_PI, False)
    lam, _ = cotangents(S)
    out = S.operator_vjp(w, mean, lam, 2, wrong=G.WRONG)
    Gt = out[None]
    flip = (-np.arange(S.nx)) % S.nx
    assert np.array_equal(Gt[:, :, 0], np.conj(Gt[:, flip, 0])) and np.abs(Gt[:, :, 0]).max() > 0
    assert np.all(Gt[:, S.M == 0] == 0) and np.all(Gt[:, 0, 0] == 0)
    # the unsymmetrised line satisfies the first condition of the definition (the same dL for every admissible dl) and not the second
    dl = S.M * G.symmetric_table(np.random.default_rng(7), S)
    one_sided = out['line_unsymmetrised']
    assert np.allclose(S.stored_pairing(one_sided, dl), S.stored_pairing(Gt, dl), rtol=1e-12, atol=0)
    assert not np.allclose(one_sided[:, :, 0], np.conj(one_sided[:, flip, 0]))


# ---------------------------------------------------------------------------------------------------- 4. wrong gradients on the GPU's inputs
WRONG_RUNS = [(run, w) for run in OC.RUNS for w in G.WRONG]


@pytest.mark.parametrize('run,wrong', WRONG_RUNS, ids=['%s-%s' % (OC.run_id(r), w) for r, w in WRONG_RUNS])
def test_the_gpu_bound_would_catch_the_wrong_gradient(run, wrong):
    """Every wrong gradient sits >= 10x the GPU bound away from the right one, in rel-L2 over the table."""
    kind, case = run
    d = OC.rel(OC.table_gradient(kind, case, wrong), OC.table_gradient(kind, case))
    print('%s %s: %.2e' % (OC.run_id(run), wrong, d))
    assert d >= 10 * OC.bound(kind), d


def test_bounds_and_measurements():
    """One measurement per run, each under its bound; the bounds are the parents' unless a measurement says otherwise, and then at most 4x
    the worst measured value."""
    assert set(OC.MEASURED) == set(OC.run_id(r) for r in OC.RUNS)
    for run in OC.RUNS:
        assert OC.MEASURED[OC.run_id(run)] < OC.bound(run[0]), run
    worst_flow = max(v for k, v in OC.MEASURED.items() if not k.startswith(('scalar', 'buoyant')))
    worst_scalar = max(v for k, v in OC.MEASURED.items() if k.startswith(('scalar', 'buoyant')))
    assert OC.BOUND_FLOW == LA.BOUND_FLOW or OC.BOUND_FLOW <= 4 * worst_flow
    assert OC.BOUND_SCALAR == LA.BOUND_SCALAR or OC.BOUND_SCALAR <= 4 * worst_scalar
    assert max(OC.BOUND_FLOW, OC.BOUND_SCALAR) < 1e-5


# ---------------------------------------------------------------------------------------------------- 5. the entry points exist
def test_the_solver_and_the_binding_have_the_operator_gradient():
    import inspect
    from nns import _lib, ops
    from nns.periodic import PeriodicSolver
    assert 'nns_spec_ns_step_operator_adjoint_f32' in set(_lib.exported_names())
    assert _lib.lib().nns_spec_ns_step_operator_adjoint_f32 is not None
    assert callable(ops.spec_ns_step_operator_adjoint_)
    for name in ('evolve', 'evolve_velocity'):
        assert 'operator' in inspect.signature(getattr(PeriodicSolver, name)).parameters
    for name in ('advance', 'advance_velocity', 'advance_scalar', 'advance_velocity_scalar'):
        assert 'operator' not in inspect.signature(getattr(PeriodicSolver, name)).parameters
    assert callable(PeriodicSolver.operator_table) and callable(PeriodicSolver.mode_table)
