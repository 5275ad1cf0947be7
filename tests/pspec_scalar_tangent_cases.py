"""Cases of the periodic solver's forward mode with a scalar (tests/test_gpu_pspec_scalar_tangent.py runs them on the GPU against
tests/pspec_scalar_tangent_oracle.py; tests/test_oracle_pspec_scalar_tangent.py checks the restatement against central differences and
against the reverse-mode restatement on the CPU and shows that the GPU bounds would catch each deliberately wrong scheme on these very inputs).

Shapes: those of pspec_linear_adjoint_cases.CASES (two column tiles with a ragged tail and a mean flow at 64x64x3, the 1 x 4 box, the 4-line
tiles of N = 1024 on either pass) and its GRID_STRIDE.  Viscosity, drag, the per-grid force, kappa, the mean gradient, the buoyancies and the
base inputs (u0, v0, theta0 with a mean) are that file's; the perturbation (dw, dtheta) and the source perturbation dforcing are further
draws of pspec_oracle.band_ic, dtheta with a mean of 0.3.  The passive and the buoyant (unstable b) step run at every shape; at 64x64x3 also
the stable buoyancy, the buoyant step with the linear terms of pspec_linear_cases.params (hyperviscosity, hypofriction, beta), the passive
one with them, and the buoyant step under the stochastic ring force."""
import functools

import numpy as np

import pspec_cases as C
import pspec_linear_adjoint_cases as LAC
import pspec_linear_adjoint_oracle as LA
import pspec_oracle as O
import pspec_scalar_adjoint_cases as SAC
import pspec_scalar_tangent_oracle as T

TWO_PI = 2 * np.pi
NU, DRAG, RHO, NSTEPS, FORCE = LAC.NU, LAC.DRAG, LAC.RHO, 3, LAC.FORCE
KAPPA, GRAD, UNSTABLE, STABLE = LAC.KAPPA, LAC.GRAD, SAC.UNSTABLE, SAC.STABLE
SEED = LAC.SEED
# the (0, 0) entry the tests put into dwhat, in units of nx ny: the step's mask must drop it, as the restatement's does
DW_00 = 0.25
# the grid mean of the scalar's perturbation: dthat's (0, 0) entry, which the step carries unchanged
DTHETA_MEAN = 0.3

CASES = list(LAC.CASES)
GRID_STRIDE = LAC.GRID_STRIDE
# kind -> (buoyancy, linear terms, stochastic ring force)
KINDS = {
    'passive': ((0.0, 0.0), False, False),
    'buoyant': (UNSTABLE, False, False),
    'buoyant-stable': (STABLE, False, False),
    'passive-linear': ((0.0, 0.0), True, False),
    'buoyant-linear': (UNSTABLE, True, False),
    'buoyant-stochastic': (UNSTABLE, False, True),
}
# (kind, case): the passive and the buoyant step at every shape, the other kinds at 64x64x3 (the case with a mean flow)
RUNS = [(k, c) for c in CASES for k in ('passive', 'buoyant')] + [(k, CASES[0]) for k in list(KINDS)[2:]]
# steps per run: NSTEPS, but 6 for the buoyant run at 1024x64, where after 3 steps theta frozen at the step's start (the nearest wrong scheme)
# lies 1.05e-5 from the right dw^, under 10x BOUND_W; after 6 steps it lies 1.88e-5 away (tests/test_oracle_pspec_scalar_tangent.py)
STEPS = {'buoyant-1024x64x2': 6}

# rel-L2 of the GPU (float32) tangent spectra (dw^, dtheta^) after steps(run) steps against the float64 oracle, per run: the worst of the call
# without dforcing, with a per-grid and with a shared one, measured on the MI355X (profiles/pspec_scalar_tangent_run.json holds the same
# figures).  BOUND_W and BOUND_T are 3-7x the worst of them, rounded; they stay under the 1e-5 target of the README and
# (tests/test_oracle_pspec_scalar_tangent.py) at least 10x under the distance of every wrong scheme where it can show.
MEASURED = {
    'passive-64x64x3': (1.56e-07, 8.27e-08),
    'buoyant-64x64x3': (1.73e-07, 8.10e-08),
    'passive-128x512x2': (1.90e-07, 7.89e-08),
    'buoyant-128x512x2': (1.79e-07, 8.05e-08),
    'passive-1024x64x2': (2.53e-07, 4.58e-08),
    'buoyant-1024x64x2': (4.29e-07, 4.46e-08),
    'passive-64x1024x2': (1.57e-07, 8.05e-08),
    'buoyant-64x1024x2': (1.57e-07, 8.06e-08),
    'buoyant-stable-64x64x3': (1.60e-07, 8.17e-08),
    'passive-linear-64x64x3': (1.55e-07, 8.02e-08),
    'buoyant-linear-64x64x3': (1.60e-07, 8.27e-08),
    'buoyant-stochastic-64x64x3': (1.74e-07, 7.92e-08),
}
BOUND_W = 1.5e-6         # 3.5x the worst (the buoyant run at 1024x64, six steps)
BOUND_T = 4e-7           # 4.8x the worst (64x64x3)
# |<J d, r> - <d, J^T r>| / (|J d| |r|) of evolve_tangent_scalar against the backward of evolve(w, n, theta=...), float64 sums on the host,
# per kind at 64x64x3, measured on the MI355X; DOT_BOUND is 3-7x the worst, rounded
DOT_KINDS = ('passive', 'buoyant', 'buoyant-linear', 'buoyant-stochastic')
DOT_MEASURED = {'passive': 3.40e-09, 'buoyant': 1.67e-10, 'buoyant-linear': 2.33e-09, 'buoyant-stochastic': 7.70e-10}
DOT_BOUND = 1.5e-8      # 4.4x the worst (passive)


def run_id(run):
    return '%s-%dx%dx%d' % ((run[0],) + run[1][:3])


def steps(run):
    return STEPS.get(run_id(run), NSTEPS)


def inputs(c):
    """dict of the float32 inputs of a case: those of pspec_linear_adjoint_cases.inputs (u0, v0 full band plus the mean, dt, the per-grid
    force (fx, fy), theta0 with a mean, the pairing fields rw, rt) and the perturbations dw, dtheta (with the mean DTHETA_MEAN) and the source
    perturbation dforcing (per grid; its first grid is the shared one), full band too."""
    nx, ny, B, Lx, Ly, mean = c
    d = dict(LAC.inputs(c))
    s = C.seed(c)
    d['dw'] = O.band_ic(B, nx, ny, s + 4000, Lx, Ly, 1.0)[0].astype(np.float32)
    d['dforcing'] = O.band_ic(B, nx, ny, s + 5000, Lx, Ly, FORCE)[0].astype(np.float32)
    d['dtheta'] = (O.band_ic(B, nx, ny, s + 6000, Lx, Ly, 1.0)[0] + DTHETA_MEAN).astype(np.float32)
    return d


def scheme(kind, c, dt, wrong=None, buoy=None, grad=GRAD):
    """The restatement of a run; buoy, grad: values that take the kind's and the file's place."""
    nx, ny, B, Lx, Ly, _ = c
    b, linear, _ = KINDS[kind]
    kw = LAC.params(c, dt) if linear else {}
    return T.ScalarTangentScheme(nx, ny, dt, RHO, NU, Lx, Ly, drag=DRAG, kappa=KAPPA, grad=grad, buoy=b if buoy is None else buoy, wrong=wrong, **kw)


def solver(kind, c, dt, drag=DRAG, buoyancy=None):
    """The PeriodicSolver of a run (GPU tests), its parameters those of scheme()."""
    from nns.periodic import PeriodicSolver
    nx, ny, B, Lx, Ly, _ = c
    b, linear, stoch = KINDS[kind]
    kw = {}
    if linear:
        pr = LAC.params(c, dt)
        kw.update(hyperviscosity=pr['hyper'], hypofriction=pr['hypo'], beta=pr['beta'])
    s = PeriodicSolver(nx, ny, dt, RHO, NU, Lx=Lx, Ly=Ly, drag=drag, kappa=KAPPA, scalar_gradient=GRAD, buoyancy=b if buoyancy is None else buoyancy, **kw)
    if stoch:
        s.ring_forcing(*LAC.ring(c), seed=SEED)
    return s


def source(c, dg):
    """The float32 source perturbation of a case: dg None: none; 'grid': one per grid [B, nx, ny]; 'shared': [1, nx, ny]."""
    d = inputs(c)['dforcing']
    return None if dg is None else d if dg == 'grid' else d[:1]


def start(S, c):
    """(w, t, mean, dw, dtheta) in rfft2 layout (complex128) of a case for the scheme S, the (0, 0) entry of dw set to DW_00 nx ny."""
    d = inputs(c)
    w, mean = S.init(d['u0'], d['v0'])
    t = S.init_scalar(d['theta0'])
    dw = np.fft.rfft2(d['dw'].astype(np.float64))
    dw[..., 0, 0] = DW_00 * c[0] * c[1]
    return w, t, mean, dw, np.fft.rfft2(d['dtheta'].astype(np.float64))


@functools.lru_cache(maxsize=None)
def oracle_tangent(run, wrong=None, dg=None, nsteps=None, buoy=None, grad=GRAD):
    """(dw^, dtheta^) after nsteps steps (None: steps(run)) in the solver's compact layout [B, my1, nx] (complex128) of the float64 scheme for the run's inputs.
    Computed once per (run, scheme, source) and shared: do not modify."""
    kind, c = run
    nsteps = steps(run) if nsteps is None else nsteps
    d = inputs(c)
    S = scheme(kind, c, d['dt'], wrong, buoy, grad)
    S.set_forcing(d['fx'], d['fy'])
    w, t, mean, dw, dth = start(S, c)
    g = source(c, dg)
    gh = None if g is None else np.fft.rfft2(g.astype(np.float64))
    starts = None
    if KINDS[kind][2]:
        starts = LA.stochastic_starts(S, LAC.amplitudes(c), SEED, w, mean, nsteps, t=t)[0]
    return tuple(S.compact(x) for x in S.step_jvp(w, t, mean, dw, dth, nsteps, dg=gh, starts=starts))


# the eigenmode of the 2 x 2 linear problem of mode m about the state at rest with the mean flow U
EIGEN = dict(nx=64, ny=64, dt=0.01, nsteps=200, nu=2e-3, kappa=5e-3, drag=0.05, b=(0.3, 1.0), G=(0.2, -1.5), U=(0.4, -0.2), m=(3, 2))
EIGEN_EXPONENT = 0.880628611


def eigenmode(t, p=EIGEN, Lx=TWO_PI, Ly=TWO_PI):
    """(dw, dtheta, Re lambda, amplitude of dw, amplitude of dtheta) at time t of the growing eigenmode of
        d/dt (dw^, dtheta^) = [[-(nu |k|^2 + drag), i (k x b)], [i (k x G) / |k|^2, -kappa |k|^2]] (dw^, dtheta^) - i (k . U) (dw^, dtheta^),
    k x b = kx by - ky bx: dw = e^(lambda t) cos phi, dtheta = c e^(lambda t) sin phi, phi = k . (x - U t), c = (nu |k|^2 + drag + lambda) / (k x b)."""
    kx, ky = TWO_PI * p['m'][0] / Lx, TWO_PI * p['m'][1] / Ly
    k2 = kx * kx + ky * ky
    kb, kg = kx * p['b'][1] - ky * p['b'][0], kx * p['G'][1] - ky * p['G'][0]
    a, d = p['nu'] * k2 + p['drag'], p['kappa'] * k2
    lam = -(a + d) / 2 + np.sqrt(((a - d) / 2) ** 2 - kb * kg / k2)
    c = (a + lam) / kb
    X, Y = np.meshgrid(Lx * np.arange(p['nx']) / p['nx'], Ly * np.arange(p['ny']) / p['ny'], indexing='ij')
    phi = kx * (X - p['U'][0] * t) + ky * (Y - p['U'][1] * t)
    g = np.exp(lam * t)
    return g * np.cos(phi), c * g * np.sin(phi), lam, g, abs(c) * g


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
