"""Full-band cases of the periodic spectral solver (tests/test_gpu_pspec_edges.py runs them on the GPU against tests/pspec_oracle.py;
tests/test_oracle_pspec.py shows on the CPU that their bounds would catch a dealiasing mask one mode too wide)."""
import numpy as np

import pspec_oracle as O

TWO_PI = 2 * np.pi
NU, RHO, UMAX, NSTEPS = 1e-3, 1.0, 1.0, 12

# (nx, ny, B, Lx, Ly, mean): every axis length 64..1024 on each axis, nx > ny and nx < ny, extreme aspect ratios, boxes != 2 pi
FULL_BAND = [
    (64, 64, 3, TWO_PI, TWO_PI, (0.3, -0.2)),
    (128, 512, 2, 1.0, 4.0, (0.0, 0.0)),
    (512, 128, 2, 5.0, 0.7, (0.0, 0.0)),
    (512, 512, 1, TWO_PI, TWO_PI, (0.0, 0.0)),
    (256, 1024, 1, TWO_PI, TWO_PI, (0.0, 0.0)),
    (1024, 256, 1, TWO_PI, TWO_PI, (0.0, 0.0)),
    (1024, 64, 2, TWO_PI, TWO_PI, (0.0, 0.0)),
    (64, 1024, 2, TWO_PI, TWO_PI, (0.0, 0.0)),
]

# rel-L2 bounds of the GPU (float32) run against the float64 oracle, for every case of FULL_BAND (and the 1024^2 x 32 grid-stride case):
# u and v, p, and the state (what against Scheme.compact(w)).  Measured on the MI355X, worst case: u, v 6.4e-7 (64x1024), p 1.5e-5
# (1024^2 x 32; 1.0e-5 at 512x128: p is a product of derivatives, the band edge weighs most), what 2.8e-7 (1024x256).  Margins 3x, 7x, 7x.
BOUND_UV, BOUND_P, BOUND_W = 2e-6, 1e-4, 2e-6


def case_id(c):
    return '%dx%d' % c[:2]


def seed(c):
    return c[0] + 3 * c[1] + c[2]


def full_band_input(nx, ny, B, Lx, Ly, mean):
    """float32 initial velocity (band_ic, max|u, v| = UMAX plus the mean) and the step dt of dt u (k_x,max + k_y,max) = 0.5."""
    u0, v0 = O.band_ic(B, nx, ny, seed((nx, ny, B)), Lx, Ly, UMAX, mean)
    dt = O.cfl_dt(nx, ny, Lx, Ly, UMAX + max(abs(m) for m in mean))
    return u0.astype(np.float32), v0.astype(np.float32), dt


def oracle_run(u0, v0, dt, nx, ny, Lx, Ly, nsteps=NSTEPS, nu=NU, widen=(0, 0)):
    """(w, (u, v, p)) of the float64 scheme after nsteps steps from (u0, v0)."""
    S = O.Scheme(nx, ny, dt, RHO, nu, Lx, Ly, widen=widen)
    w, mean = S.init(u0, v0)
    w = S.step(w, mean, nsteps)
    return w, S.fields(w, mean)
