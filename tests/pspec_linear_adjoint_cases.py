"""Cases of the reverse mode of the periodic solver's linear step -- hyperviscosity, hypofriction and beta, with or without the scalar, buoyancy
and the white-in-time ring force (tests/test_gpu_pspec_linear_adjoint.py runs them on the GPU against tests/pspec_linear_adjoint_oracle.py;
tests/test_oracle_pspec_linear_adjoint.py checks the restatement against central differences on the CPU and shows that the GPU bounds would
catch each deliberately wrong scheme on these very inputs).

Shapes: those of pspec_linear_cases.CASES (two column tiles with a ragged tail, the 1 x 4 box's anisotropic wavenumbers, the 4-line tiles of
N = 1024, my1 = 342).  Linear terms: pspec_linear_cases.params as they stand (nu_h K^8 dt = 5 at the band's corner, 0.05 per step of
hypofriction and 0.2 rad per step of beta on the gravest mode): over NSTEPS = 3 steps every wrong scheme of the restatement is then at
least 339x the GPU bound away from the right gradient (stage_shift at 64x64x3; the nearest mistake in the factors themselves, an E^2 turned
by the angle of E at 64x1024, 2460x), so beta did not have to be raised.  Viscosity, drag, the per-grid force, the scalar and the buoyancy
are those of the two parent adjoint case files."""
import functools

import numpy as np

import pspec_adjoint_cases as AC
import pspec_cases as C
import pspec_linear_adjoint_oracle as A
import pspec_linear_cases as LC
import pspec_oracle as O
import pspec_scalar_adjoint_cases as SAC
import pspec_stochastic_cases as XC
import pspec_stochastic_oracle as ST

TWO_PI = 2 * np.pi
NU, DRAG, RHO, NSTEPS, FORCE = AC.NU, AC.DRAG, AC.RHO, 3, AC.FORCE
KAPPA, GRAD, BUOY = SAC.KAPPA, SAC.GRAD, SAC.UNSTABLE
SEED = XC.SEED

# (nx, ny, B, Lx, Ly, mean)
CASES = list(LC.CASES)
assert [c[:3] for c in CASES] == [(64, 64, 3), (128, 512, 2), (1024, 64, 2), (64, 1024, 2)] and CASES[1][3:5] == (1.0, 4.0)
KINDS = ('flow', 'scalar', 'buoyant', 'stochastic')
# (kind, case): the flow at every shape; the scalar, the buoyant and the stochastic step at 64x64x3
RUNS = [('flow', c) for c in CASES] + [(k, CASES[0]) for k in KINDS[1:]]
GRID_STRIDE = (1024, 64, 400, TWO_PI, TWO_PI, (0.0, 0.0))       # 400 x 22 columns in 4-line tiles: more tiles than the launch has workgroups

# the project's bounds for these quantities: the flow adjoint's for (wbar, gbar), the scalar adjoint's for (wbar, thetabar, gbar)
BOUND_FLOW, BOUND_SCALAR = AC.BOUND, SAC.BOUND


def bound(kind):
    return BOUND_SCALAR if kind in ('scalar', 'buoyant') else BOUND_FLOW


# rel-L2 of the GPU (float32) gradients after NSTEPS steps against the float64 oracle, per run: (wbar, gbar), with a scalar (wbar, thetabar,
# gbar), measured on the MI355X (profiles/pspec_linear_adjoint_run.json holds the same figures)
MEASURED = {
    'flow-64x64x3': (1.37e-7, 1.06e-7),
    'flow-128x512x2': (1.75e-7, 1.22e-7),
    'flow-1024x64x2': (2.75e-7, 1.58e-7),
    'flow-64x1024x2': (4.34e-7, 2.20e-7),
    'scalar-64x64x3': (1.40e-7, 1.16e-7, 1.11e-7),
    'buoyant-64x64x3': (1.42e-7, 1.33e-7, 1.11e-7),
    'stochastic-64x64x3': (1.29e-7, 1.07e-7),
}
# No measured error exceeds a starting bound (the worst, wbar of the flow at 64x1024, is 9.2x under BOUND_FLOW; with a scalar 21x under
# BOUND_SCALAR), so both bounds are the parents', unchanged.  evolve_velocity of the buoyant run at 64x64x3 measured 1.8e-7 (u0, v0), 1.7e-7
# (theta0) and 1.3e-7 (forcing); a table of nu and drag alone against the existing adjoints 5.0e-8 (flow) and 5.9e-8 (buoyant), the bound from
# the factors' roundings being 5.2e-7; a stochastic rollout in two chunks against the uncut call 1.8e-7 (w) and 1.8e-7 (gradient), linear and
# forced alike -- not the same bits, because the state crosses the cut as a field.


def run_id(run):
    return '%s-%dx%dx%d' % ((run[0],) + run[1][:3])


def params(c, dt):
    """dict(hyper, hypo, beta) of a case: pspec_linear_cases.params."""
    nx, ny, B, Lx, Ly, _ = c
    return LC.params(nx, ny, Lx, Ly, dt)


def inputs(c):
    """dict of the float32 inputs of a case: u0, v0 (full band, plus the mean), dt, the per-grid force (fx, fy), the scalar theta0 (full band,
    plus a mean of 0.25) and the cotangent fields rw, rt of the vorticity and of the scalar after NSTEPS steps (full band; rt with a mean)."""
    nx, ny, B, Lx, Ly, mean = c
    u0, v0, dt = C.full_band_input(nx, ny, B, Lx, Ly, mean)
    s = C.seed(c)
    f32 = lambda a: a.astype(np.float32)
    fx, fy = O.band_ic(B, nx, ny, s + 1000, Lx, Ly, FORCE)
    rw, rt = O.band_ic(B, nx, ny, s + 2000, Lx, Ly, 1.0)
    theta0 = O.band_ic(B, nx, ny, s + 3000, Lx, Ly, 1.0)[0] + 0.25
    return dict(u0=u0, v0=v0, dt=dt, fx=f32(fx), fy=f32(fy), theta0=f32(theta0), rw=f32(rw), rt=f32(rt + 0.1))


def scheme(kind, c, dt, wrong=None, linear=True):
    """The restatement of a run; linear = False: nu_h = mu = beta = 0."""
    nx, ny, B, Lx, Ly, _ = c
    kw = params(c, dt) if linear else {}
    if kind in ('scalar', 'buoyant'):
        kw.update(kappa=KAPPA, grad=GRAD)
    if kind == 'buoyant':
        kw['buoy'] = BUOY
    return A.LinearAdjointScheme(nx, ny, dt, RHO, NU, Lx, Ly, drag=DRAG, wrong=wrong, **kw)


def solver(kind, c, dt, linear=True, **kw):
    """The PeriodicSolver of a run (GPU tests), its parameters those of scheme(); 'stochastic' adds the ring force of ring()."""
    from nns.periodic import PeriodicSolver
    nx, ny, B, Lx, Ly, _ = c
    if linear:
        pr = params(c, dt)
        kw.update(hyperviscosity=pr['hyper'], hypofriction=pr['hypo'], beta=pr['beta'])
    if kind in ('scalar', 'buoyant'):
        kw.update(kappa=KAPPA, scalar_gradient=GRAD)
    if kind == 'buoyant':
        kw['buoyancy'] = BUOY
    s = PeriodicSolver(nx, ny, dt, RHO, NU, Lx=Lx, Ly=Ly, drag=DRAG, **kw)
    if kind == 'stochastic':
        s.ring_forcing(*ring(c), seed=SEED)
    return s


@functools.lru_cache(maxsize=None)
def ring(c):
    """(rate, k_lo, k_hi) of the stochastic run: kicks of the state's size, as pspec_stochastic_cases.traj_rate makes them (over NSTEPS steps
    they put in, in the mean, the energy the initial state holds), on the ring of pspec_stochastic_cases.traj_ring."""
    nx, ny, B, Lx, Ly, _ = c
    d = inputs(c)
    S = scheme('flow', c, d['dt'])
    w0, _ = S.init(d['u0'], d['v0'])
    return (XC.traj_rate(S, w0, NSTEPS),) + tuple(XC.traj_ring(nx, ny, Lx, Ly))


def amplitudes(c):
    nx, ny, B, Lx, Ly, _ = c
    rate, k_lo, k_hi = ring(c)
    return ST.amplitude_table(nx, ny, Lx, Ly, ST.ring_rates(nx, ny, Lx, Ly, rate, k_lo, k_hi))


@functools.lru_cache(maxsize=None)
def oracle_gradient(kind, c, wrong=None, nsteps=NSTEPS, linear=True):
    """(wbar, gbar), with a scalar (wbar, thetabar, gbar), in the solver's compact layout [B, my1, nx] (complex128) of the float64 scheme for
    the run's inputs: the cotangents of the start spectra and of g^ for L = sum w(x, nsteps dt) rw(x) (+ theta(x, nsteps dt) rt(x)).  Computed
    once per (run, scheme) and shared: do not modify."""
    d = inputs(c)
    S = scheme(kind, c, d['dt'], wrong if wrong in A.WRONG else None, linear)
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    f64 = lambda a: np.fft.rfft2(a.astype(np.float64))
    if kind == 'stochastic':
        out = A.stochastic_vjp(S, amplitudes(c), SEED, w, mean, f64(d['rw']), nsteps, wrong=wrong if wrong in A.WRONG_STOCHASTIC else None)
    elif kind == 'flow':
        out = S.step_vjp(w, mean, f64(d['rw']), nsteps)
    else:
        out = S.step_vjp(w, mean, f64(d['rw']), nsteps, t=S.init_scalar(d['theta0']), mu=f64(d['rt']))
    return tuple(S.compact(g) for g in out)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
