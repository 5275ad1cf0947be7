"""Cases of the periodic solver's forward mode (tests/test_gpu_pspec_tangent.py runs them on the GPU against tests/pspec_tangent_oracle.py;
tests/test_oracle_pspec_tangent.py checks the restatement against central differences and against the reverse-mode restatements on the CPU
and shows that the GPU bound would catch each deliberately wrong scheme on these very inputs).

Shapes: those of pspec_adjoint_cases.CASES (every axis length 64 ... 1024 on both passes, the 64-line and the 4-line tiles) and its GRID_STRIDE;
viscosity, drag, the per-grid force and the pairing field r are that file's, the base inputs pspec_cases.full_band_input.  The perturbation
dw and the source perturbation dforcing are further draws of pspec_oracle.band_ic.  One linear run takes the hyperviscosity, hypofriction
and beta of pspec_linear_cases.params, one stochastic run the ring and the rate of pspec_stochastic_cases (through
pspec_linear_adjoint_cases.ring, which makes the kicks as large as the state)."""
import functools

import numpy as np

import pspec_adjoint_cases as AC
import pspec_cases as C
import pspec_linear_adjoint_cases as LAC
import pspec_linear_adjoint_oracle as LA
import pspec_linear_cases as LC
import pspec_oracle as O
import pspec_stochastic_cases as XC
import pspec_tangent_oracle as T

TWO_PI = 2 * np.pi
NU, DRAG, RHO, NSTEPS, FORCE = AC.NU, AC.DRAG, AC.RHO, 3, AC.FORCE
SEED = XC.SEED
# the (0, 0) entry the tests put into the tangent spectrum they hand to the step, in units of nx ny (a grid mean of the perturbation): the
# step's mask must drop it, as the restatement's does
DW_00 = 0.25

CASES = list(AC.CASES)
GRID_STRIDE = AC.GRID_STRIDE
KINDS = ('forced', 'linear', 'stochastic')
# (kind, case): the forced step at every shape; the linear and the stochastic step at 64x64x3 (the case with a mean flow)
RUNS = [('forced', c) for c in CASES] + [(k, CASES[0]) for k in KINDS[1:]]

# rel-L2 of the GPU (float32) tangent spectrum after NSTEPS steps against the float64 oracle, per run: (without dforcing, dforcing per grid,
# dforcing shared), measured on the MI355X (profiles/pspec_tangent_run.json holds the same figures).  BOUND is 3-7x the worst of them,
# rounded; it stays under the 1e-5 target of the README and (tests/test_oracle_pspec_tangent.py) at least 10x under the distance of every
# wrong scheme.
MEASURED = {
    'forced-64x64x3': (1.53e-07, 1.53e-07, 1.56e-07),
    'forced-128x512x2': (1.77e-07, 1.89e-07, 1.90e-07),
    'forced-512x128x2': (1.70e-07, 1.68e-07, 1.74e-07),
    'forced-256x256x1': (2.13e-07, 2.46e-07, 2.46e-07),
    'forced-1024x64x2': (2.26e-07, 2.53e-07, 2.52e-07),
    'forced-64x1024x2': (1.57e-07, 1.50e-07, 1.49e-07),
    'linear-64x64x3': (1.45e-07, 1.52e-07, 1.55e-07),
    'stochastic-64x64x3': (1.50e-07, 1.53e-07, 1.53e-07),
}
BOUND = 1e-6           # 4.0x the worst (a per-grid source at 1024x64)
# |sum dw_out r - (sum w.grad dw + sum forcing.grad dforcing)| / (|dw_out| |r|) of evolve_tangent against the backward of evolve, float64 sums
# on the host, per kind at 64x64x3, measured on the MI355X; DOT_BOUND is 3-7x the worst, rounded
DOT_MEASURED = {'forced': 6.65e-9, 'linear': 1.57e-8, 'stochastic': 6.60e-10}
DOT_BOUND = 8e-8       # 5.1x the worst (linear)


def run_id(run):
    return '%s-%dx%dx%d' % ((run[0],) + run[1][:3])


def inputs(c):
    """dict of the float32 inputs of a case: those of pspec_adjoint_cases.inputs (u0, v0 full band plus the mean, dt, the per-grid force
    (fx, fy), the pairing field r) and the vorticity perturbation dw and the source perturbation dforcing (per grid; its first grid is the
    shared one), full band too."""
    nx, ny, B, Lx, Ly, mean = c
    d = dict(AC.inputs(c))
    s = C.seed(c)
    d['dw'] = O.band_ic(B, nx, ny, s + 4000, Lx, Ly, 1.0)[0].astype(np.float32)
    d['dforcing'] = O.band_ic(B, nx, ny, s + 5000, Lx, Ly, FORCE)[0].astype(np.float32)
    return d


def params(kind, c, dt):
    """dict(hyper, hypo, beta) of a run: pspec_linear_cases.params for the linear one, nothing for the others."""
    nx, ny, B, Lx, Ly, _ = c
    return LC.params(nx, ny, Lx, Ly, dt) if kind == 'linear' else {}


def scheme(kind, c, dt, wrong=None):
    nx, ny, B, Lx, Ly, _ = c
    return T.TangentScheme(nx, ny, dt, RHO, NU, Lx, Ly, drag=DRAG, wrong=wrong, **params(kind, c, dt))


def solver(kind, c, dt, drag=DRAG):
    """The PeriodicSolver of a run (GPU tests), its parameters those of scheme(); 'stochastic' adds the ring force."""
    from nns.periodic import PeriodicSolver
    nx, ny, B, Lx, Ly, _ = c
    pr = params(kind, c, dt)
    kw = dict(hyperviscosity=pr['hyper'], hypofriction=pr['hypo'], beta=pr['beta']) if pr else {}
    s = PeriodicSolver(nx, ny, dt, RHO, NU, Lx=Lx, Ly=Ly, drag=drag, **kw)
    if kind == 'stochastic':
        s.ring_forcing(*LAC.ring(c), seed=SEED)
    return s


def source(c, dg):
    """The float32 source perturbation of a case: dg None: none; 'grid': one per grid [B, nx, ny]; 'shared': [1, nx, ny]."""
    d = inputs(c)['dforcing']
    return None if dg is None else d if dg == 'grid' else d[:1]


@functools.lru_cache(maxsize=None)
def oracle_tangent(run, wrong=None, dg=None, nsteps=NSTEPS):
    """dw^ after nsteps steps in the solver's compact layout [B, my1, nx] (complex128) of the float64 scheme for the run's inputs, the (0, 0)
    entry of the input set to DW_00 nx ny.  Computed once per (run, scheme, source) and shared: do not modify."""
    kind, c = run
    d = inputs(c)
    S = scheme(kind, c, d['dt'], wrong)
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    dw = np.fft.rfft2(d['dw'].astype(np.float64))
    dw[..., 0, 0] = DW_00 * c[0] * c[1]
    g = source(c, dg)
    gh = None if g is None else np.fft.rfft2(g.astype(np.float64))
    starts = None
    if kind == 'stochastic':
        starts = LA.stochastic_starts(S, LAC.amplitudes(c), SEED, w, mean, nsteps)[0]
    return S.compact(S.step_jvp(w, mean, dw, nsteps, dg=gh, starts=starts))


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
