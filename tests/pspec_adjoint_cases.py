"""Cases of the periodic solver's reverse mode (tests/test_gpu_pspec_adjoint.py runs them on the GPU against tests/pspec_adjoint_oracle.py;
tests/test_oracle_pspec_adjoint.py checks the restatement against central differences on the CPU and shows that the GPU bound would catch
each deliberately wrong scheme on these very inputs)."""
import functools

import numpy as np

import pspec_adjoint_oracle as A
import pspec_cases as C
import pspec_oracle as O

TWO_PI = 2 * np.pi
NU, DRAG, RHO, NSTEPS = 5e-3, 0.5, 1.0, 3
FORCE = 0.5            # max |f| of the per-grid force

# (nx, ny, B, Lx, Ly, mean): every axis length 64..1024 on both passes; 66 columns in 64-line tiles (64x64x3), 4-line tiles at 1024
CASES = [
    (64, 64, 3, TWO_PI, TWO_PI, (0.3, -0.2)),
    (128, 512, 2, 1.0, 4.0, (0.0, 0.0)),
    (512, 128, 2, 5.0, 0.7, (0.0, 0.0)),
    (256, 256, 1, TWO_PI, TWO_PI, (0.0, 0.0)),
    (1024, 64, 2, TWO_PI, TWO_PI, (0.0, 0.0)),
    (64, 1024, 2, TWO_PI, TWO_PI, (0.0, 0.0)),
]
GRID_STRIDE = (1024, 64, 400, TWO_PI, TWO_PI, (0.0, 0.0))       # 400 x 22 columns in 4-line tiles: more tiles than the launch has workgroups

# rel-L2 of the GPU (float32) gradients after NSTEPS steps against the float64 oracle, per case (wbar, gbar), measured on the MI355X
# (profiles/pspec_adjoint_run.json holds the same figures).  BOUND is 3-7x the worst of them, rounded; it stays under the 1e-5 target of the
# README and (tests/test_oracle_pspec_adjoint.py) at least 10x under the distance of every wrong scheme.
MEASURED = {
    '64x64x3': (1.33e-7, 1.14e-7),
    '128x512x2': (2.91e-7, 1.76e-7),
    '512x128x2': (6.42e-7, 3.03e-7),
    '256x256x1': (2.43e-7, 1.46e-7),
    '1024x64x2': (3.17e-7, 1.80e-7),
    '64x1024x2': (8.79e-7, 3.85e-7),
}
BOUND = 4e-6           # 4.6x the worst (wbar at 64x1024); advance_velocity at 64x64x3 measured 1.8e-7 (u0, v0) and 1.2e-7 (forcing)


def case_id(c):
    return '%dx%dx%d' % c[:3]


def inputs(c):
    """dict of the float32 inputs of a case: u0, v0 (full band, plus the mean), dt, the per-grid force (fx, fy) and the cotangent field r of the
    vorticity after NSTEPS steps (full band too: the u of another draw)."""
    nx, ny, B, Lx, Ly, mean = c
    u0, v0, dt = C.full_band_input(nx, ny, B, Lx, Ly, mean)
    s = C.seed(c)
    fx, fy = O.band_ic(B, nx, ny, s + 1000, Lx, Ly, FORCE)
    r = O.band_ic(B, nx, ny, s + 2000, Lx, Ly, 1.0)[0]
    return dict(u0=u0, v0=v0, dt=dt, fx=fx.astype(np.float32), fy=fy.astype(np.float32), r=r.astype(np.float32))


def scheme(c, dt, wrong=None):
    nx, ny, B, Lx, Ly, mean = c
    return A.AdjointScheme(nx, ny, dt, RHO, NU, Lx, Ly, drag=DRAG, wrong=wrong)


@functools.lru_cache(maxsize=None)
def oracle_gradient(c, wrong=None, nsteps=NSTEPS):
    """(wbar, gbar) in the solver's compact layout [B, my1, nx] (complex128) of the float64 scheme for the case's inputs: the cotangents of
    the start spectrum and of g^ for L = sum w(x, NSTEPS dt) r(x).  Computed once per (case, scheme) and shared: do not modify."""
    d = inputs(c)
    S = scheme(c, d['dt'], wrong)
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    wbar, gbar = S.step_vjp(w, mean, np.fft.rfft2(d['r'].astype(np.float64)), nsteps)
    return S.compact(wbar), S.compact(gbar)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
