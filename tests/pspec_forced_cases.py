"""Forced cases of the periodic spectral solver: the full-band inputs of tests/pspec_cases.py under a Kolmogorov force and a linear drag
(tests/test_gpu_pspec_forced.py runs them on the GPU against tests/pspec_forced_oracle.py; tests/test_oracle_pspec_forced.py shows on
the CPU that their bounds would catch a build that ignores the force, the drag, or applies the force in one stage only)."""
import numpy as np

import pspec_cases as C
import pspec_forced_oracle as F
import pspec_oracle as O

# Kolmogorov wavenumber, force amplitude and drag of every forced case.  The runs are 12 steps at the CFL step of pspec_cases (t = 0.01 ..
# 0.1 at max|u| = 1): the force moves u by ~ AMP t and the drag by ~ DRAG t |u|, both >= 1e-2 relative -- 5000x pspec_cases.BOUND_UV.
KF, AMP, DRAG = 4, 2.0, 1.0


def scheme(nx, ny, dt, Lx, Ly, drag=DRAG, nu=C.NU, **kw):
    return F.ForcedScheme(nx, ny, dt, C.RHO, nu, Lx, Ly, drag=drag, **kw)


def oracle_run(S, u0, v0, nsteps=C.NSTEPS):
    """(w, (u, v, p)) of the float64 scheme S (its force already set) after nsteps steps from (u0, v0)."""
    w, mean = S.init(u0, v0)
    w = S.step(w, mean, nsteps)
    return w, S.fields(w, mean)


def random_forces(B, nx, ny, seed, Lx, Ly, amp=AMP):
    """B different solenoidal forces filling the whole kept band (band_ic with another seed), max|f| = amp, float32."""
    fx, fy = O.band_ic(B, nx, ny, seed, Lx, Ly, amp)
    return fx.astype(np.float32), fy.astype(np.float32)


def rough_force(nx, ny, seed, amp=AMP):
    """A force that is neither solenoidal nor band-limited nor zero-mean: independent random fx, fy spectra over every wavenumber
    (amplitude 1 / (1 + |m|^2)) plus a mean, scaled to max|f| = amp, float32 [1, nx, ny]."""
    rng = np.random.default_rng(seed)
    mx, my = np.fft.fftfreq(nx) * nx, np.arange(ny // 2 + 1)
    a = 1.0 / (1.0 + mx[:, None] ** 2 + my[None, :] ** 2)
    spec = (rng.standard_normal((2, 1, nx, ny // 2 + 1)) + 1j * rng.standard_normal((2, 1, nx, ny // 2 + 1))) * a
    f = np.fft.irfft2(spec, s=(nx, ny))
    f *= amp / np.abs(f).max()
    return (f[0] + 0.3 * amp).astype(np.float32), (f[1] - 0.2 * amp).astype(np.float32)
