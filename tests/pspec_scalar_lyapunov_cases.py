"""Cases of K tangent pairs on one base with a scalar and of their Lyapunov spectrum (tests/test_gpu_pspec_scalar_lyapunov.py runs them on
the GPU against tests/pspec_scalar_lyapunov_oracle.py; tests/test_oracle_pspec_scalar_lyapunov.py checks the restatement on the CPU and shows
that the GPU bounds would catch each deliberately wrong spectrum on these very inputs).

Shapes, kinds, runs and base inputs are those of pspec_scalar_tangent_cases (CASES, KINDS, RUNS, GRID_STRIDE, inputs); member k's dw and
dtheta are further draws of pspec_oracle.band_ic with seed + 4000 + 100 k and seed + 6000 + 100 k (dtheta with the mean DTHETA_MEAN), so that
member 0 is that file's pair."""
import functools

import numpy as np

import pspec_cases as C
import pspec_linear_adjoint_cases as LAC
import pspec_linear_adjoint_oracle as LA
import pspec_oracle as O
import pspec_scalar_lyapunov_oracle as SLY
import pspec_scalar_tangent_cases as TC
import pspec_scalar_tangent_oracle as T
from pspec_scalar_tangent_cases import CASES, KINDS, RUNS, GRID_STRIDE, inputs          # noqa: F401

TWO_PI = 2 * np.pi
K_BITWISE, NSTEPS_BITWISE = 3, 3                  # GPU test 1
K_SPECTRUM, NSTEPS, EVERY = 3, 6, 2               # GPU test 11
K_ORTHO = 4                                       # GPU tests 9 and 10
WEIGHT = 4.0                                      # the scalar_weight != 1 of the tests
# the nearly dependent set of pspec_lyapunov_cases, applied to the pair: d_k = d_0 + NEAR NEAR_AMP e_k, both halves
NEAR, NEAR_AMP = 1e-3, 1e-2
SPECTRUM_KINDS = ('passive', 'buoyant', 'buoyant-linear', 'buoyant-stochastic')
SPECTRUM_RUNS = [(k, CASES[0]) for k in SPECTRUM_KINDS]
EIGEN = TC.EIGEN                                  # the base at rest (GPU test 12): its K = 4 vectors are rest_fields()
REST_EVERY = 50

# Figures of the GPU run on the MI355X against the float64 oracle or the analytic value, and their bounds: 3-7x the worst measured figure,
# rounded.  The exponents' figure is |lambda_gpu - lambda_ref| nsteps dt, the error of the summed logs; the logs' is |log R_kk - its reference|.
MEASURED = {
    'gram': 1.64e-15,              # max |G - G_numpy| / max |G_numpy| of the variance Gram and of the pair's at weight 1 and 4 (float64 sums in another order)
    # max |G - I| after orthonormalize_tangents_scalar, K = 4 random pairs (weight 1, 4), and after lyapunov_spectrum_scalar on the runs of GPU test 11
    'ortho_random': {'random-w1': 1.48e-08, 'random-w4': 1.35e-08, 'passive': 1.27e-08, 'buoyant': 1.36e-08, 'buoyant-linear': 1.09e-08,
                     'buoyant-stochastic': 1.28e-08, 'buoyant-w4': 1.55e-08},
    'ortho_near': {'w1': 1.82e-08, 'w4': 1.51e-08},      # the same on the nearly dependent set
    # max |log R_kk - oracle|, the oracle on the GPU's own float32 spectra
    'logs': {'random-w1': 7.43e-09, 'random-w4': 6.84e-09, 'near-w1': 9.74e-09, 'near-w4': 8.73e-09},
    'spectrum': {'passive': 5.97e-08, 'buoyant': 6.70e-08, 'buoyant-linear': 5.38e-08, 'buoyant-stochastic': 4.99e-08, 'buoyant-w4': 3.80e-08},
    'rest': {'w1': 4.81e-07, 'w4': 1.19e-07},            # against the analytic (lambda_+, lambda_+, lambda_-, lambda_-)
    'single': {'w1': 2.97e-08, 'w4': 5.00e-08},          # K = 1 against lyapunov_exponent_scalar, the same inputs
}
BOUND = {
    'gram': 8e-15,                 # 4.9x
    'ortho_random': 8e-8,          # 5.2x the worst (after the buoyant run at weight 4)
    'ortho_near': 9e-8,            # 4.9x the worst (weight 1)
    'logs': 5e-8,                  # 5.1x the worst (the nearly dependent set, weight 1)
    'spectrum': 3e-7,              # 4.5x the worst (buoyant)
    'rest': 2e-6,                  # 4.2x the worst (weight 1)
    'single': 2.5e-7,              # 5.0x the worst (weight 4)
}
# The diagonal of the variance Gram matrix against spec_ns_scalar_diag's variance has no figure: both kernels walk a grid in the same order and
# add wt (x x + y y) of the same values, so the two float64 sums are the same bits, and the test asks for that.
# The restatement's own error on the base at rest, max |lambda - analytic| nsteps dt at weight 1 and 4: RK4's truncation over 200 steps of
# dt = 0.01 (tests/test_oracle_pspec_scalar_lyapunov.py measures, prints and bounds it by 1e-8)
REST_ORACLE = 4.66e-10


def tangent_fields(c, K):
    """(dw, dtheta), float32 [K, B, nx, ny] each: the perturbations of a case; member 0 is pspec_scalar_tangent_cases.inputs(c)'s pair."""
    nx, ny, B, Lx, Ly, mean = c
    s = C.seed(c)
    dw = np.stack([O.band_ic(B, nx, ny, s + 4000 + 100 * k, Lx, Ly, 1.0)[0] for k in range(K)]).astype(np.float32)
    dth = np.stack([O.band_ic(B, nx, ny, s + 6000 + 100 * k, Lx, Ly, 1.0)[0] + TC.DTHETA_MEAN for k in range(K)]).astype(np.float32)
    return dw, dth


def near_fields(c, K):
    """The nearly dependent set d_k = d_0 + NEAR NEAR_AMP e_k (k >= 1) of tangent_fields' members, both halves of the pair."""
    out = []
    for e in tangent_fields(c, K):
        e = e.astype(np.float64)
        d = e[:1] + NEAR * NEAR_AMP * e
        d[0] = e[0]
        out.append(d.astype(np.float32))
    return tuple(out)


def spectra(S, fields):
    """complex128 rfft2 spectra (dw^, dtheta^) of float32 field pairs, masked as init_tangents_scalar masks them."""
    dw, dth = fields
    return S.M * np.fft.rfft2(np.asarray(dw, dtype=np.float64)), S.Mt * np.fft.rfft2(np.asarray(dth, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def oracle_spectrum(run, wrong=None, weight=1.0, K=K_SPECTRUM, nsteps=NSTEPS, every=EVERY):
    """float64 [B, K]: the finite-time exponents of the float64 scheme for the run's inputs.  Computed once per (run, variant): do not modify."""
    kind, c = run
    d = TC.inputs(c)
    S = TC.scheme(kind, c, d['dt'])
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    t = S.init_scalar(d['theta0'])
    starts = None
    if KINDS[kind][2]:
        starts = LA.stochastic_starts(S, LAC.amplitudes(c), TC.SEED, w, mean, nsteps, t=t)[0]
    return SLY.ScalarLyapunov(S, weight, wrong).exponents(w, t, mean, *spectra(S, tangent_fields(c, K)), nsteps, every, starts)[0]


@functools.lru_cache(maxsize=None)
def oracle_logs(wrong=None, near=False, weight=1.0, K=K_ORTHO):
    """float64 [B, K]: log diag R of the factorisation of the random (near: the nearly dependent) set at CASES[0]."""
    c = CASES[0]
    S = TC.scheme('buoyant', c, TC.inputs(c)['dt'])
    return SLY.ScalarLyapunov(S, weight, wrong).qr(*spectra(S, (near_fields if near else tangent_fields)(c, K)))[2]


def rest_rates(p=EIGEN, Lx=TWO_PI, Ly=TWO_PI):
    """(lambda_+, lambda_-, c_+, c_-) of the 2 x 2 linear problem of pspec_scalar_tangent_cases.eigenmode: lambda_+- = -(a + d) / 2 +- sqrt(...),
    c = (a + lambda) / (k x b) the amplitude of dtheta beside dw's 1."""
    kx, ky = TWO_PI * p['m'][0] / Lx, TWO_PI * p['m'][1] / Ly
    k2 = kx * kx + ky * ky
    kb, kg = kx * p['b'][1] - ky * p['b'][0], kx * p['G'][1] - ky * p['G'][0]
    a, d = p['nu'] * k2 + p['drag'], p['kappa'] * k2
    root = np.sqrt(((a - d) / 2) ** 2 - kb * kg / k2)
    lp, lm = -(a + d) / 2 + root, -(a + d) / 2 - root
    return lp, lm, (a + lp) / kb, (a + lm) / kb


def rest_fields(p=EIGEN, Lx=TWO_PI, Ly=TWO_PI):
    """(dw, dtheta), float64 [4, 1, nx, ny] each: grow-cos, grow-sin, decay-cos, decay-sin -- the lambda_+ eigenmode (dw = cos phi, dtheta =
    c sin phi) at the phases phi and phi + pi / 2, then the same for lambda_-.  Each pair is orthogonal and of equal norm by translation
    invariance and spans an invariant plane, and the four span the wavevector's whole invariant subspace: the finite-time spectrum is
    (lambda_+, lambda_+, lambda_-, lambda_-) for any scalar_weight."""
    lp, lm, cp, cm = rest_rates(p, Lx, Ly)
    kx, ky = TWO_PI * p['m'][0] / Lx, TWO_PI * p['m'][1] / Ly
    X, Y = np.meshgrid(Lx * np.arange(p['nx']) / p['nx'], Ly * np.arange(p['ny']) / p['ny'], indexing='ij')
    phi = kx * X + ky * Y
    dw = [np.cos(phi), -np.sin(phi), np.cos(phi), -np.sin(phi)]
    dth = [cp * np.sin(phi), cp * np.cos(phi), cm * np.sin(phi), cm * np.cos(phi)]
    return np.stack(dw)[:, None], np.stack(dth)[:, None]


def rest_scheme(p=EIGEN):
    return T.ScalarTangentScheme(p['nx'], p['ny'], p['dt'], 1.0, p['nu'], drag=p['drag'], kappa=p['kappa'], grad=p['G'], buoy=p['b'])


@functools.lru_cache(maxsize=None)
def oracle_rest(weight=1.0, wrong=None, nsteps=None):
    """float64 [4]: the restatement's finite-time spectrum on the base at rest with the mean flow U."""
    p = EIGEN
    S = rest_scheme(p)
    z = np.zeros((1, p['nx'], p['ny'] // 2 + 1), dtype=np.complex128)
    mean = np.array([p['U']], dtype=np.float64)
    dw, dth = rest_fields(p)
    return SLY.ScalarLyapunov(S, weight, wrong).exponents(z, z.copy(), mean, np.fft.rfft2(dw), np.fft.rfft2(dth),
                                                            p['nsteps'] if nsteps is None else nsteps, REST_EVERY)[0][0]
