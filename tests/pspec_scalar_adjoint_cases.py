"""Cases of the reverse mode of the periodic solver's scalar and buoyant step (tests/test_gpu_pspec_scalar_adjoint.py runs them on the GPU
against tests/pspec_scalar_adjoint_oracle.py; tests/test_oracle_pspec_scalar_adjoint.py checks the restatement against central differences on
the CPU and shows that the GPU bound would catch each deliberately wrong scheme on these very inputs)."""
import functools

import numpy as np

import pspec_cases as C
import pspec_oracle as O
import pspec_scalar_adjoint_oracle as A

TWO_PI = 2 * np.pi
NU, DRAG, KAPPA, RHO, NSTEPS = 5e-3, 0.5, 2e-3, 1.0, 3
GRAD = (0.7, -0.4)
FORCE = 0.5            # max |f| of the per-grid force
UNSTABLE, STABLE, PASSIVE = (0.6, 1.5), (0.6, -1.5), (0.0, 0.0)       # b . G = -0.18 (convection), +1.02 (internal waves), no buoyancy

# (nx, ny, B, Lx, Ly, mean, b): 66 columns in 64-line tiles with a mean flow (64x64x3), once buoyant and once passive; both passes on a
# stretched box; 4-line tiles and the longest lines of each pass at 1024; b . G of either sign across the buoyant cases
CASES = [
    (64, 64, 3, TWO_PI, TWO_PI, (0.3, -0.2), UNSTABLE),
    (64, 64, 3, TWO_PI, TWO_PI, (0.3, -0.2), PASSIVE),
    (128, 512, 2, 1.0, 4.0, (0.0, 0.0), STABLE),
    (512, 128, 2, 5.0, 0.7, (0.0, 0.0), UNSTABLE),
    (1024, 64, 2, TWO_PI, TWO_PI, (0.0, 0.0), STABLE),
    (64, 1024, 2, TWO_PI, TWO_PI, (0.0, 0.0), UNSTABLE),
]
# 374 x 22 columns in 4-line tiles = 2057 tiles, the launch has at most 2048 workgroups; 372 grids (2046 tiles) would fit, and the grids come in pairs
GRID_STRIDE = (1024, 64, 374, TWO_PI, TWO_PI, (0.0, 0.0), UNSTABLE)

# rel-L2 of the GPU (float32) gradients after NSTEPS steps against the float64 oracle, per case (wbar, thetabar, gbar), measured on the MI355X
# (profiles/pspec_scalar_adjoint_run.json holds the same figures).  BOUND is 3-7x the worst of them, rounded; it stays under the 1e-5 target
# of the README and (tests/test_oracle_pspec_scalar_adjoint.py) at least 10x under the distance of every wrong scheme.
MEASURED = {
    '64x64x3-unstable': (1.30e-7, 1.41e-7, 1.09e-7),
    '64x64x3-passive': (1.44e-7, 1.36e-7, 1.12e-7),
    '128x512x2-stable': (1.65e-7, 1.21e-7, 1.25e-7),
    '512x128x2-unstable': (6.19e-7, 1.17e-7, 3.52e-7),
    '1024x64x2-stable': (2.98e-7, 1.31e-7, 1.80e-7),
    '64x1024x2-unstable': (8.36e-7, 8.47e-8, 3.88e-7),
}
# 3.6x the worst (wbar at 64x1024); the nearest wrong scheme (no_gradient at 64x1024) is 3.98e-5 away, 13x the bound; advance_velocity_scalar at
# 64x64x3 measured 1.7e-7 (u0, v0), 1.8e-7 (theta0) and 1.2e-7 (forcing)
BOUND = 3e-6


def case_id(c):
    return '%dx%dx%d-%s' % (c[:3] + ({UNSTABLE: 'unstable', STABLE: 'stable', PASSIVE: 'passive'}[c[6]],))


def inputs(c):
    """dict of the float32 inputs of a case: u0, v0 (full band, plus the mean), dt, the per-grid force (fx, fy), the scalar theta0 (full band,
    plus a mean of 0.25) and the cotangent fields rw, rt of the vorticity and of the scalar after NSTEPS steps (full band too; rt with a mean)."""
    nx, ny, B, Lx, Ly, mean, _ = c
    u0, v0, dt = C.full_band_input(nx, ny, B, Lx, Ly, mean)
    s = C.seed(c)
    f32 = lambda a: a.astype(np.float32)
    fx, fy = O.band_ic(B, nx, ny, s + 1000, Lx, Ly, FORCE)
    rw, rt = O.band_ic(B, nx, ny, s + 2000, Lx, Ly, 1.0)
    theta0 = O.band_ic(B, nx, ny, s + 3000, Lx, Ly, 1.0)[0] + 0.25
    return dict(u0=u0, v0=v0, dt=dt, fx=f32(fx), fy=f32(fy), theta0=f32(theta0), rw=f32(rw), rt=f32(rt + 0.1))


def scheme(c, dt, wrong=None):
    nx, ny, B, Lx, Ly, mean, buoy = c
    return A.ScalarAdjointScheme(nx, ny, dt, RHO, NU, Lx, Ly, drag=DRAG, kappa=KAPPA, grad=GRAD, buoy=buoy, wrong=wrong)


@functools.lru_cache(maxsize=None)
def oracle_gradient(c, wrong=None, nsteps=NSTEPS):
    """(wbar, thetabar, gbar) in the solver's compact layout [B, my1, nx] (complex128) of the float64 scheme for the case's inputs: the
    cotangents of the start spectra and of g^ for L = sum w(x, NSTEPS dt) rw(x) + theta(x, NSTEPS dt) rt(x).  Computed once per (case, scheme)
    and shared: do not modify."""
    d = inputs(c)
    S = scheme(c, d['dt'], wrong)
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    t = S.init_scalar(d['theta0'])
    f64 = lambda a: np.fft.rfft2(a.astype(np.float64))
    return tuple(S.compact(g) for g in S.step_vjp(w, t, mean, f64(d['rw']), f64(d['rt']), nsteps))


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
