"""Passive-scalar cases of the periodic spectral solver: five of the full-band inputs of tests/pspec_cases.py, under the Kolmogorov force and
drag of tests/pspec_forced_cases.py, carrying a scalar that fills the whole kept band (tests/test_gpu_pspec_scalar.py runs them on the GPU
against tests/pspec_scalar_oracle.py; tests/test_oracle_pspec_scalar.py shows on the CPU that their bound would catch a wrong diffusivity, an
ignored gradient, a dragged scalar, a velocity frozen over the stages and a mask one mode too wide)."""
import numpy as np

import pspec_cases as C
import pspec_forced_cases as FC
import pspec_oracle as O
import pspec_scalar_oracle as SO

# the smallest shapes that cover both partial column tiles (3 * 22 = 66 columns in tiles of 64), the 4-line tiles of N = 1024 on each axis,
# nx != ny and boxes != 2 pi; the first has a mean flow
CASES = [C.FULL_BAND[k] for k in (0, 1, 2, 6, 7)]
assert [c[:3] for c in CASES] == [(64, 64, 3), (128, 512, 2), (512, 128, 2), (1024, 64, 2), (64, 1024, 2)]
NSTEPS = 12
KAPPA, GRAD = 2e-3, (0.7, -0.4)
# the analytic advected sine, 200 steps: (nx, ny, Lx, Ly, m, U, kappa, dt); RK4's error is n (omega dt)^5 / 120 of the amplitude, omega = k . U:
# 4.0e-8, 2e-8 and 1e-8
SINES = [
    (64, 64, C.TWO_PI, C.TWO_PI, (3, 5), (0.5, 0.3), 0.01, 0.01),
    (256, 1024, C.TWO_PI, 2 * C.TWO_PI, (20, -20), (0.5, -0.3), 1e-3, 0.002),
    (1024, 64, 1.0, C.TWO_PI, (-2, 10), (-0.4, 0.4), 1e-3, 0.0025),
]
# Their mean c and gradient G (the solution is sin(k . (x - U t)) exp(-kappa |k|^2 t) + c - t G . U) are sized by float32: the device keeps
# the mean as the (0, 0) coefficient, and adding a constant increment to a float32 value rounds the same way every time, up to half an ulp
# (2^-25 relative to the value) per stage update and 800 updates in 200 steps -- a drift of up to 2.4e-5 |mean|, inherent to the format
# (measured on the MI355X with c = 0.5, G = (0.7, -0.4): 2.1e-6, 5.0e-6, 1.3e-5 for the three cases, linear in the step count, against
# <= 1.5e-6 for the fluctuation).  With |mean| <= 1.05e-2 throughout, that term is below a quarter of the 2e-6 bound at amplitude >= 0.5;
# c = 0.005 and G = GRAD / 100 keep |mean| <= 7.2e-3 while the gradient still moves the mean by t G . U = 4.6e-3, 1.9e-3, 2.2e-3:
# >= 950x the bound, so a gradient ignored or misapplied is caught.
SINE_STEPS, SINE_MEAN, SINE_GRAD = 200, 0.005, (GRAD[0] / 100, GRAD[1] / 100)


def scalar_input(nx, ny, B, Lx, Ly, mean):
    """float32 scalar [B, nx, ny] filling the whole kept band: max|theta - 0.5| = 1 around a mean of 0.5."""
    th = np.fft.irfft2(O.band_psi(B, nx, ny, 1000 + C.seed((nx, ny, B))), s=(nx, ny))
    return (th / np.abs(th).max() + 0.5).astype(np.float32)


def scheme(nx, ny, dt, Lx, Ly, forced=True, **kw):
    """The restatement of a case: forced = the Kolmogorov force and drag of pspec_forced_cases, else the unforced flow."""
    kw.setdefault('kappa', KAPPA)
    kw.setdefault('grad', GRAD)
    S = SO.ScalarScheme(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG if forced else 0.0, **kw)
    return S.kolmogorov_forcing(FC.KF, FC.AMP) if forced else S


def rel_l2c(a, b):
    """rel-L2 of complex (or real) arrays: conftest.rel_l2 casts to float64 and would drop the imaginary parts."""
    a, b = np.asarray(a), np.asarray(b)
    d = np.linalg.norm(b.ravel())
    return np.linalg.norm((a - b).ravel()) / (d if d > 0 else 1.0)


def oracle_run(S, u0, v0, th0, nsteps=NSTEPS):
    """(w, t, mean) of the float64 scheme S after nsteps steps."""
    w, mean = S.init(u0, v0)
    w, t = S.step(w, S.init_scalar(th0), mean, nsteps)
    return w, t, mean


_RUNS = {}


def reference(case):
    """(S, u0, v0, th0, w, t, mean): a case under the force and drag after NSTEPS steps of the restatement; computed once per session, shared
    by the tests that need it and read-only."""
    if case not in _RUNS:
        nx, ny, B, Lx, Ly, mean = case
        u0, v0, dt = C.full_band_input(*case)
        th0 = scalar_input(*case)
        S = scheme(nx, ny, dt, Lx, Ly)
        w, t, m = oracle_run(S, u0, v0, th0)
        for a in (u0, v0, th0, w, t, m):
            a.setflags(write=False)
        _RUNS[case] = (S, u0, v0, th0, w, t, m)
    return _RUNS[case]
