"""Buoyant cases of the periodic spectral solver: the five full-band shapes, force, drag, kappa and G of tests/pspec_scalar_cases.py with the
scalar acting on the flow through b = (0.3, 1.2) (tests/test_gpu_pspec_buoyant.py runs them on the GPU against tests/pspec_buoyant_oracle.py;
tests/test_oracle_pspec_buoyant.py shows on the CPU that their bounds would catch a buoyancy of the wrong sign, with swapped components, left
out, frozen over the stages, or missing from the pressure), and the analytic plane waves."""
import numpy as np

import pspec_buoyant_oracle as BO
import pspec_cases as C
import pspec_forced_cases as FC
import pspec_scalar_cases as SC

# the shapes of pspec_scalar_cases: both partial column tiles, the 4-line tiles of N = 1024 on each axis, nx != ny and boxes != 2 pi
CASES = SC.CASES
NSTEPS = SC.NSTEPS
assert NSTEPS == 12
KAPPA, GRAD, BUOY = SC.KAPPA, SC.GRAD, (0.3, 1.2)
# the pressure of a buoyant state against the restatement, rel-L2: 3.6x the worst figure measured on the MI355X over the five cases, 1.26e-6 at
# 128 x 512 (profiles/pspec_buoyant_run.json; tests/test_gpu_pspec_buoyant.py::test_buoyant_pressure_against_the_oracle lists them); the
# 'p_without_b' mutation is judged against the same number
BOUND_P = 4.5e-6

# the analytic plane waves (BO.plane_wave), 200 steps: (nx, ny, Lx, Ly, m, b, G, nu = kappa, dt), vorticity amplitude 1.  The mean flow is
# U = 0.5 (Gy, -Gx) / |G|: G . U = 0, so the mean of theta has no constant source (the float32 drift pspec_scalar_cases.py explains).
# The last repeats the first with G reversed: unstable, compared with cosh(omega t).
WAVES = [
    (64, 64, C.TWO_PI, C.TWO_PI, (3, 5), (0.0, 2.0), (0.0, 1.5), 0.01, 0.01),
    (256, 1024, C.TWO_PI, 2 * C.TWO_PI, (20, -20), (0.6, 2.0), (0.45, 1.5), 1e-3, 0.002),
    (1024, 64, 1.0, C.TWO_PI, (-2, 10), (2.0, 0.6), (1.5, 0.45), 1e-3, 0.0025),
    (64, 64, C.TWO_PI, C.TWO_PI, (3, 5), (0.0, 2.0), (0.0, -1.5), 0.01, 0.01),
]
WAVE_IDS = ['%dx%d%s' % (w[0], w[1], '-unstable' if w[5][0] * w[6][0] + w[5][1] * w[6][1] < 0 else '') for w in WAVES]
WAVE_STEPS = 200


def wave_flow(G):
    """The mean flow of a wave case: 0.5 (Gy, -Gx) / |G|."""
    g = np.hypot(G[0], G[1])
    return (0.5 * G[1] / g, -0.5 * G[0] / g)


def wave_rk4_error(wave, U, nsteps=WAVE_STEPS, dt=None):
    """RK4's error after nsteps steps as a fraction of the amplitude: n ((omega + |k . U|) dt)^5 / 120."""
    nx, ny, Lx, Ly, m, b, G, nu, dt0 = wave
    dt = dt0 if dt is None else dt
    kx, ky = 2 * np.pi * m[0] / Lx, 2 * np.pi * m[1] / Ly
    om = BO.plane_wave(nx, ny, 0.0, m, b, G, U, nu, Lx, Ly)[6]
    return nsteps * ((om + abs(kx * U[0] + ky * U[1])) * dt) ** 5 / 120


def scheme(nx, ny, dt, Lx, Ly, forced=True, **kw):
    """The restatement of a case: forced = the Kolmogorov force and drag of pspec_forced_cases, else the unforced flow."""
    kw.setdefault('kappa', KAPPA)
    kw.setdefault('grad', GRAD)
    kw.setdefault('buoy', BUOY)
    S = BO.BuoyantScheme(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG if forced else 0.0, **kw)
    return S.kolmogorov_forcing(FC.KF, FC.AMP) if forced else S


def oracle_run(S, u0, v0, th0, nsteps=NSTEPS):
    """(w, t, mean) of the float64 scheme S after nsteps steps."""
    w, mean = S.init(u0, v0)
    w, t = S.step(w, S.init_scalar(th0), mean, nsteps)
    return w, t, mean


_RUNS = {}


def reference(case):
    """(S, u0, v0, th0, w, t, mean): a case under the force, drag and buoyancy after NSTEPS steps of the restatement; computed once per session,
    shared by the tests that need it and read-only.  The inputs are those of pspec_scalar_cases."""
    if case not in _RUNS:
        nx, ny, B, Lx, Ly, mean = case
        u0, v0, dt = C.full_band_input(*case)
        th0 = SC.scalar_input(*case)
        S = scheme(nx, ny, dt, Lx, Ly)
        w, t, m = oracle_run(S, u0, v0, th0)
        for a in (u0, v0, th0, w, t, m):
            a.setflags(write=False)
        _RUNS[case] = (S, u0, v0, th0, w, t, m)
    return _RUNS[case]
