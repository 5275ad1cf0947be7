"""Cases of the periodic solver's reverse mode in its linear operator (tests/test_gpu_pspec_operator_grad.py runs them on the GPU against
tests/pspec_operator_grad_oracle.py; tests/test_oracle_pspec_operator_grad.py checks the restatement against central differences on the CPU
and shows that the GPU bounds would catch each deliberately wrong gradient on these very inputs).

Shapes, inputs, parameters and runs are those of tests/pspec_linear_adjoint_cases.py as they stand: 64x64x3, 128x512x2 on the 1 x 4 box (two
column tiles with a ragged tail), 1024x64x2, 64x1024x2 and GRID_STRIDE; the flow at every shape, the scalar, the buoyant and the stochastic
run at 64x64x3; NSTEPS = 3; nu_h K^8 dt = 5 at the band's corner, so the stiffest mode has l = -2.5 and E^2 = e^-5: the products
c conj(D) there are formed without dividing by it."""
import functools

import numpy as np

import pspec_linear_adjoint_cases as LA
import pspec_operator_grad_oracle as G

NSTEPS = LA.NSTEPS
CASES, RUNS, GRID_STRIDE, KINDS = LA.CASES, LA.RUNS, LA.GRID_STRIDE, LA.KINDS
run_id, inputs, rel = LA.run_id, LA.inputs, LA.rel
PARAMETERS = ('nu', 'drag', 'nu_h', 'mu', 'beta')

# The starting bounds are the parents', for the same kind of quantity (a float32 cotangent after NSTEPS steps against the float64 scheme).
# The table's gradient is a sum of products of two such quantities (a cotangent and a stage state) over 3 stages and NSTEPS steps; see MEASURED.
BOUND_FLOW, BOUND_SCALAR = LA.BOUND_FLOW, LA.BOUND_SCALAR


def bound(kind):
    return BOUND_SCALAR if kind in ('scalar', 'buoyant') else BOUND_FLOW


# rel-L2 over the table of the GPU (float32) gradient in the operator after NSTEPS steps against the float64 oracle, per run, measured on the
# MI355X (profiles/pspec_operator_grad_run.json holds the same figures)
MEASURED = {
    'flow-64x64x3': 1.55e-7,
    'flow-128x512x2': 1.43e-7,
    'flow-1024x64x2': 1.90e-7,
    'flow-64x1024x2': 1.31e-7,
    'scalar-64x64x3': 1.85e-7,
    'buoyant-64x64x3': 2.02e-7,
    'stochastic-64x64x3': 1.44e-7,
}
# No measured error exceeds a starting bound (the worst, the buoyant run's 2.0e-7, is 15x under BOUND_SCALAR; the flow's worst 21x under
# BOUND_FLOW), so both bounds are the parents', unchanged; every wrong gradient of the restatement lies >= 37x the bound away
# (line_unsymmetrised at 64x1024, where the line is 1 row of 342: 1.5e-4 against 4e-6; the nearest other mistake, stage_shift, 1.4e-2).  The five scalar gradients through operator_table at
# 64x64x3, each relative to its own size: nu 3.9e-8, drag 9.9e-8, nu_h 2.7e-7, mu 1.4e-6, beta 2.0e-7 (mu's is a sum with cancellation: 0.24
# against terms of the size of drag's 2.3); evolve_velocity of the buoyant run 1.9e-7; a table of nu and drag alone on a solver without the
# linear terms against ``advance`` 1.1e-7 forward and gradient (bound 5.2e-7 from the factors' roundings).


def scheme(kind, c, dt):
    """The restatement of a run: pspec_linear_adjoint_cases.scheme's parameters on an OperatorGradScheme."""
    nx, ny, B, Lx, Ly, _ = c
    kw = LA.params(c, dt)
    if kind in ('scalar', 'buoyant'):
        kw.update(kappa=LA.KAPPA, grad=LA.GRAD)
    if kind == 'buoyant':
        kw['buoy'] = LA.BUOY
    return G.OperatorGradScheme(nx, ny, dt, LA.RHO, LA.NU, Lx, Ly, drag=LA.DRAG, **kw)


@functools.lru_cache(maxsize=None)
def oracle_gradient(kind, c, nsteps=NSTEPS):
    """(S, dict): the scheme of the run and, by None (the right one) and by every name of pspec_operator_grad_oracle.WRONG, the gradient in
    the table PER GRID in the rfft2 layout [B, nx, nh] (complex128) of L = sum w(x, nsteps dt) rw(x) (+ theta(x, nsteps dt) rt(x)) for the
    run's inputs.  Computed once per run, all schemes in one sweep, and shared: do not modify."""
    d = inputs(c)
    S = scheme(kind, c, d['dt'])
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    f64 = lambda a: np.fft.rfft2(a.astype(np.float64))
    if kind == 'stochastic':
        out = G.stochastic_operator_vjp(S, LA.amplitudes(c), LA.SEED, w, mean, f64(d['rw']), nsteps, wrong=G.WRONG)
    elif kind == 'flow':
        out = S.operator_vjp(w, mean, f64(d['rw']), nsteps, wrong=G.WRONG)
    else:
        out = S.operator_vjp(w, mean, f64(d['rw']), nsteps, t=S.init_scalar(d['theta0']), mu=f64(d['rt']), wrong=G.WRONG)
    return S, out


def table_gradient(kind, c, wrong=None):
    """The gradient in the solver's table [my1, nx] (complex128: Re, Im the derivatives in Re l, Im l): the grids summed."""
    S, out = oracle_gradient(kind, c)
    return S.compact(out[wrong].sum(axis=0))


def parameter_gradients(kind, c):
    """dict name -> d L / d parameter through the table's formula: sum over the stored entries of G . d l / d parameter."""
    S, out = oracle_gradient(kind, c)
    Gt = out[None].sum(axis=0)
    return {k: float(S.stored_pairing(Gt, dl)) for k, dl in S.parameter_derivatives().items()}
