"""Cases of the periodic solver's second-order adjoint (tests/test_gpu_pspec_second_adjoint.py runs them on the GPU against
tests/pspec_second_adjoint_oracle.py; tests/test_oracle_pspec_second_adjoint.py checks the restatement against central differences of the
reverse-mode restatement on the CPU and shows that the GPU bound would catch each deliberately wrong scheme on these very inputs).

Shapes: those of pspec_adjoint_cases.CASES and its GRID_STRIDE.  Kinds and runs: those of pspec_tangent_cases (the forced step at every
shape; the linear and the stochastic step at 64x64x3, the case with a mean flow).  Inputs: those of pspec_tangent_cases.inputs (the base,
the per-grid force, the perturbation dw, the source perturbation dforcing, the pairing field r, which is the cotangent lam) plus a second
pairing field r2, a further draw of pspec_oracle.band_ic.  Two settings of the cotangent's derivative: 'generic', dlam = r2, and 'pure',
dlam = 0, which leaves the term a Gauss-Newton product drops and nothing else."""
import functools

import numpy as np

import pspec_cases as C
import pspec_linear_adjoint_cases as LAC
import pspec_linear_adjoint_oracle as LA
import pspec_oracle as O
import pspec_second_adjoint_oracle as S2
import pspec_tangent_cases as TC

NU, DRAG, RHO, NSTEPS, SEED = TC.NU, TC.DRAG, TC.RHO, TC.NSTEPS, TC.SEED
CASES = list(TC.CASES)
GRID_STRIDE = TC.GRID_STRIDE
KINDS = TC.KINDS
RUNS = list(TC.RUNS)
SETTINGS = ('generic', 'pure')
run_id = TC.run_id
rel = TC.rel

# rel-L2 of the GPU (float32) dwbar and dgbar after NSTEPS steps against the float64 oracle, per run and setting: (dwbar, dgbar), each the worst
# over dforcing none / per grid / shared, measured on the MI355X (profiles/pspec_second_adjoint_run.json holds the same figures).  BOUND, per
# setting, is 3-7x the worst of them, rounded; it stays under the 1e-5 target of the README and (tests/test_oracle_pspec_second_adjoint.py) at
# least 10x under the distance of every wrong scheme where that scheme can show.  The 'pure' setting is the harder one for the kernels -- the
# first-order share that 'generic' adds is the better conditioned part -- and the sharper one for the mutations: in 'generic' the two schemes that
# only misplace the tangent stages (stage_shift_d, frozen_tangent) lie 26x and 52x the bound away at 64x64x3, 22x and 45x at 256x256 and 13.6x
# and 28x at 64x1024, but 1.4x ... 2.9x and 2.9x ... 5.9x at 128x512, 512x128 and 1024x64 (HIDDEN_IN_GENERIC), where the first-order share hides
# them; there the 'pure' setting carries them (>= 6.7e-3, 740x its bound), as wrong_shows says.
MEASURED = {
    ('forced-64x64x3', 'generic'): (1.93e-07, 1.61e-07),
    ('forced-64x64x3', 'pure'): (3.38e-07, 3.29e-07),
    ('forced-128x512x2', 'generic'): (2.20e-07, 1.85e-07),
    ('forced-128x512x2', 'pure'): (9.29e-07, 9.25e-07),
    ('forced-512x128x2', 'generic'): (4.38e-07, 3.16e-07),
    ('forced-512x128x2', 'pure'): (1.22e-06, 1.45e-06),
    ('forced-256x256x1', 'generic'): (2.31e-07, 1.82e-07),
    ('forced-256x256x1', 'pure'): (4.43e-07, 4.31e-07),
    ('forced-1024x64x2', 'generic'): (3.76e-07, 2.72e-07),
    ('forced-1024x64x2', 'pure'): (1.09e-06, 1.16e-06),
    ('forced-64x1024x2', 'generic'): (1.17e-06, 5.30e-07),
    ('forced-64x1024x2', 'pure'): (2.66e-06, 2.64e-06),
    ('linear-64x64x3', 'generic'): (1.73e-07, 1.57e-07),
    ('linear-64x64x3', 'pure'): (3.15e-07, 2.98e-07),
    ('stochastic-64x64x3', 'generic'): (1.95e-07, 1.66e-07),
    ('stochastic-64x64x3', 'pure'): (3.23e-07, 3.13e-07),
}
BOUND = {'generic': 5e-6,      # 4.3x the worst (dwbar at 64x1024)
         'pure': 9e-6}         # 3.4x the worst (dwbar at 64x1024)
# |<a, H b> - <b, H a>| / (|a| |H b|) through hessian_vector_product with l = 1/2 sum (w_N - obs)^2, jointly in (w, forcing), float64 sums on
# the host, per kind at 64x64x3, measured on the MI355X; SYM_BOUND is 3-7x the worst, rounded
SYM_MEASURED = {'forced': 4.66e-9, 'linear': 1.18e-8, 'stochastic': 5.94e-9}
SYM_BOUND = 6e-8       # 5.1x the worst (linear)


HIDDEN_IN_GENERIC = [c for c in CASES if c[:2] in ((128, 512), (512, 128), (1024, 64))]      # the shapes of MEASURED's note


def wrong_shows(run, setting, wrong):
    """Whether a wrong scheme of pspec_second_adjoint_oracle.WRONG can show in a run and setting, at >= 10x the bound: mean_in_du needs a mean
    flow (the 64x64x3 case), not_conjugated the complex factors of the linear run; the two schemes that misplace the tangent stages show in
    the 'pure' setting everywhere and in 'generic' at every shape but the three of HIDDEN_IN_GENERIC (MEASURED's note)."""
    kind, c = run
    if wrong == 'mean_in_du':
        return c[5] != (0.0, 0.0)
    if wrong == 'not_conjugated':
        return kind == 'linear'
    if wrong in ('stage_shift_d', 'frozen_tangent'):
        return setting == 'pure' or c not in HIDDEN_IN_GENERIC
    return True


def inputs(c):
    """dict of the float32 inputs of a case: those of pspec_tangent_cases.inputs and the second pairing field r2 (full band)."""
    nx, ny, B, Lx, Ly, mean = c
    d = dict(TC.inputs(c))
    d['r2'] = O.band_ic(B, nx, ny, C.seed(c) + 6000, Lx, Ly, 1.0)[0].astype(np.float32)
    return d


def scheme(kind, c, dt, wrong=None):
    nx, ny, B, Lx, Ly, _ = c
    return S2.SecondAdjointScheme(nx, ny, dt, RHO, NU, Lx, Ly, drag=DRAG, wrong=wrong, **TC.params(kind, c, dt))


solver = TC.solver


@functools.lru_cache(maxsize=None)
def fields(c):
    """dict of the float32 FIELDS both sides start from, so that no init of the solver's sits between the restatement and the kernels: the
    vorticity w of (u0, v0) and the vorticity source g of the force (fx, fy), both from the float64 restatement and rounded to float32, the
    mean flow, and the inputs' dw, dforcing, r, r2 and dt as they are.  Computed once per case and shared: do not modify."""
    d = inputs(c)
    S = scheme('forced', c, d['dt'])
    w, mean = S.init(d['u0'], d['v0'])
    g = S.init(d['fx'], d['fy'])[0]
    f32 = lambda spectrum: S.irfft2(spectrum).astype(np.float32)
    return dict(dt=d['dt'], w=f32(w), mean=mean.astype(np.float32), g=f32(g), dw=d['dw'], dforcing=d['dforcing'], r=d['r'], r2=d['r2'])


def dforcing(c, dg):
    """The float32 source perturbation of a case: dg None: none; 'grid': one per grid [B, nx, ny]; 'shared': [1, nx, ny] (the first grid's)."""
    d = fields(c)['dforcing']
    return None if dg is None else d if dg == 'grid' else d[:1]


@functools.lru_cache(maxsize=None)
def oracle_second(run, setting, wrong=None, dg=None, nsteps=NSTEPS):
    """(wbar, gbar, dwbar, dgbar) as fields [B, nx, ny] (float64), the form PeriodicSolver hands them out in, of the float64 scheme for the run's fields():
    lam = r, dlam = r2 ('generic') or 0 ('pure'), the direction (dw, dforcing as ``dg`` names it).  Computed once per (run, setting, scheme,
    source) and shared: do not modify."""
    kind, c = run
    d = fields(c)
    S = scheme(kind, c, d['dt'], wrong)
    f64 = lambda a: S.M * np.fft.rfft2(a.astype(np.float64))
    w, mean = f64(d['w']), d['mean'].astype(np.float64)
    S.g = f64(d['g'])
    g = dforcing(c, dg)
    starts = None
    if kind == 'stochastic':
        starts = LA.stochastic_starts(S, LAC.amplitudes(c), SEED, w, mean, nsteps)[0]
    out = S.step_second_vjp(w, mean, f64(d['dw']), None if g is None else f64(g), f64(d['r']), f64(d['r2']) if setting == 'generic' else None,
                            nsteps, starts=starts)
    return tuple(S.irfft2(x) for x in out[:4])
