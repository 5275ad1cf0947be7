"""Stochastic-forcing cases of the periodic spectral solver (tests/test_gpu_pspec_stochastic.py runs them on the GPU against
tests/pspec_stochastic_oracle.py; tests/test_oracle_pspec_stochastic.py shows on the CPU that their bounds would catch a kick without sqrt(dt),
with variance 1 per component, with an unconjugated j = 0 mirror, or applied before the step)."""
import numpy as np

import pspec_buoyant_cases as BC
import pspec_cases as C
import pspec_forced_cases as FC
import pspec_forced_oracle as F
import pspec_oracle as O
import pspec_scalar_cases as SC
import pspec_stochastic_oracle as ST

SEED = 0x5EED0123456789AB                 # both key words non-zero; the moments of its samples are recorded in test_oracle_pspec_stochastic.py
TWO_PI = C.TWO_PI

# ---- one step from rest is the kick itself: (nx, ny, B, Lx, Ly), the smallest shapes at which the kernel's indexing can go wrong:
# two column tiles with a ragged tail (3 * 22 = 66 columns in tiles of 64); the 4-line tiles of N = 1024; my1 = 342; an elongated box with many
# shells; and the grid-stride loop (400 * 22 = 8800 columns > 2048 tiles x 4 lines)
KICKS = [
    (64, 64, 3, TWO_PI, TWO_PI),
    (1024, 64, 2, TWO_PI, TWO_PI),
    (64, 1024, 2, TWO_PI, TWO_PI),
    (128, 512, 2, 1.0, 4.0),
    (1024, 64, 400, TWO_PI, TWO_PI),
]
KICK_IDS = ['%dx%d-B%d' % k[:3] for k in KICKS]
KICK_DT, KICK_RATE = 0.01, 1.0
# relative to a_k sqrt(dt) max(1, |xi_k|): about 4.5 float32 ulp from logf, sqrtf, sincospif and two products at |xi| <= 4.08, with ~2x margin
KICK_TOL = 2e-6


def kick_ring(nx, ny, B, Lx, Ly):
    """(k_lo, k_hi) of a kick case: the middle half of the longer axis's band, so the ring crosses every column tile of that axis and leaves
    modes inside and outside it on every line; the batch of 400 gets a thin ring (the oracle's Philox runs in NumPy integers)."""
    K = max(TWO_PI / Lx * ((nx - 1) // 3), TWO_PI / Ly * (O.kept_y(ny) - 1))
    return (0.30 * K, 0.36 * K) if B > 16 else (0.25 * K, 0.75 * K)


def kick_table(case):
    """The float32 table [my1, nx] of a kick case (the oracle's builder)."""
    nx, ny, B, Lx, Ly = case
    return ST.amplitude_table(nx, ny, Lx, Ly, ST.ring_rates(nx, ny, Lx, Ly, KICK_RATE, *kick_ring(*case)))


def kick_samples(case, mutate=None):
    """(mask [my1, nx], xi [B, M]): the forced stored modes of a kick case and the oracle's samples of step 0 on them, ids = arange(B)."""
    nx, ny, B, Lx, Ly = case
    mask = kick_table(case) != 0
    return mask, ST.xi_stored(nx, ny, SEED, 0, np.arange(B), mutate, where=mask)[:, mask]


def moments(xi):
    """(mean |xi|^2 - 1, |mean xi|, 5 / sqrt(M)) of M samples: both are within the last for a complex standard normal, at 5 standard deviations."""
    xi = np.asarray(xi).ravel()
    return float(np.mean(np.abs(xi) ** 2) - 1.0), float(np.abs(np.mean(xi))), 5.0 / np.sqrt(xi.size)


# ---- trajectories: NSTEPS steps of the full-band inputs under the Kolmogorov force and drag of pspec_forced_cases plus a ring force
NSTEPS = C.NSTEPS
TRAJ = [C.FULL_BAND[k] for k in (0, 1, 6)]
assert [c[:3] for c in TRAJ] == [(64, 64, 3), (128, 512, 2), (1024, 64, 2)]
TRAJ_IDS = [C.case_id(c) for c in TRAJ]
SCALAR_CASE, BUOYANT_CASE = SC.CASES[0], BC.CASES[0]
assert SCALAR_CASE[:3] == (64, 64, 3) and BUOYANT_CASE[:3] == (64, 64, 3)


def traj_ring(nx, ny, Lx, Ly):
    """(k_lo, k_hi): |k| between 4 and 6 fundamental wavenumbers of the shorter side (shells 4..6 on the 2 pi box)."""
    k1 = max(TWO_PI / Lx, TWO_PI / Ly)
    return 4 * k1, 6 * k1


def traj_rate(S, w0, nsteps=NSTEPS):
    """The ring's injection rate: the kicks of the whole run put in as much energy, in the mean, as the initial state holds (batch mean of the
    fluctuation energy), so the noise is comparable to the state and not a perturbation of it."""
    return float(np.mean(S.diag(w0)[0]) / (nsteps * S.dt))


_RUNS = {}


def reference(kind, case):
    """kind 'flow' (TRAJ), 'scalar', 'buoyant': (S, X, inputs, w, t or None, mean, ratio): the float64 scheme, its stochastic stepper, the float32
    inputs (u0, v0[, th0]), the state after NSTEPS steps and the ratio of the energy the kicks inject in the mean to the initial energy
    (1 by construction of traj_rate; printed by the tests).  Computed once per session, shared and read-only."""
    key = (kind, case)
    if key not in _RUNS:
        nx, ny, B, Lx, Ly, _ = case
        u0, v0, dt = C.full_band_input(*case)
        if kind == 'flow':
            S, th0 = FC.scheme(nx, ny, dt, Lx, Ly).kolmogorov_forcing(FC.KF, FC.AMP), None
        else:
            S, th0 = (SC if kind == 'scalar' else BC).scheme(nx, ny, dt, Lx, Ly), SC.scalar_input(*case)
        w0, mean = S.init(u0, v0)
        rate = traj_rate(S, w0)
        amp = ST.amplitude_table(nx, ny, Lx, Ly, ST.ring_rates(nx, ny, Lx, Ly, rate, *traj_ring(nx, ny, Lx, Ly)))
        X = ST.Stochastic(S, amp, SEED)
        if th0 is None:
            w, t = X.step(w0, mean, NSTEPS), None
        else:
            w, t = X.step(w0, mean, NSTEPS, t=S.init_scalar(th0))
        ratio = float(ST.injection(nx, ny, Lx, Ly, amp).sum() * NSTEPS * dt / np.mean(S.diag(w0)[0]))
        ins = (u0, v0) if th0 is None else (u0, v0, th0)
        for a in ins + (w, mean, amp) + (() if t is None else (t,)):
            a.setflags(write=False)
        _RUNS[key] = (S, X, ins, w, t, mean, rate, ratio)
    return _RUNS[key]


# ---- statistics from rest (nu = 0, no drag, 64 x 64, ring shells 4..6)
REST = (64, 64, TWO_PI, TWO_PI)
REST_RING, REST_RATE, REST_DT = (4.0, 6.0), 0.5, 0.01


def rest_scheme():
    nx, ny, Lx, Ly = REST
    return F.ForcedScheme(nx, ny, REST_DT, C.RHO, 0.0, Lx, Ly)


def rest_table():
    nx, ny, Lx, Ly = REST
    return ST.amplitude_table(nx, ny, Lx, Ly, ST.ring_rates(nx, ny, Lx, Ly, REST_RATE, *REST_RING))


def stored_count(amp):
    """The stored modes that are forced."""
    return int(np.count_nonzero(amp))
