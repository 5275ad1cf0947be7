"""Cases of K tangents on one base and of the Lyapunov spectrum (tests/test_gpu_pspec_lyapunov.py runs them on the GPU against
tests/pspec_lyapunov_oracle.py; tests/test_oracle_pspec_lyapunov.py checks the restatement on the CPU and shows that the GPU bounds would
catch each deliberately wrong spectrum on these very inputs).

Shapes, runs and base inputs are those of pspec_tangent_cases (CASES, RUNS, GRID_STRIDE, inputs); tangent k's dw is a further draw of
pspec_oracle.band_ic with seed + 4000 + 100 k, so that k = 0 is that file's dw."""
import functools

import numpy as np

import pspec_cases as C
import pspec_linear_adjoint_cases as LAC
import pspec_linear_adjoint_oracle as LA
import pspec_lyapunov_oracle as LY
import pspec_oracle as O
import pspec_tangent_cases as TC
from pspec_tangent_cases import CASES, RUNS, GRID_STRIDE, inputs          # noqa: F401

TWO_PI = 2 * np.pi
K_BITWISE, NSTEPS_BITWISE = 3, TC.NSTEPS          # GPU test 1
K_SPECTRUM, NSTEPS, EVERY = 3, 6, 2               # GPU test 8
K_ORTHO = 4                                       # GPU test 7
# the nearly dependent set: d_k = d_0 + NEAR e_k, e_k tangent k's own draw at NEAR_AMP of d_0's amplitude.  The members then differ by 1e-5 of
# their size (some 170 float32 ulps) and the Gram matrix has a condition number near 1e11: the first Cholesky pass leaves an error near 1e-5
# in the logs and in the orthogonality, which is what the second pass is for -- and what makes its logs visible to a test (a set apart by
# 1e-3 leaves 2e-9, under float32 round-off)
NEAR, NEAR_AMP = 1e-3, 1e-2
SPECTRUM_RUNS = [(k, CASES[0]) for k in TC.KINDS]

# The base at rest (GPU test 9): w = 0, a mean flow, drag; four single modes with |m|^2 = 2, 1, 5, 4 in that order, and the pair A + B, A - B
# of |m|^2 = 1 and 4.  nu |k|^2 nsteps dt = 0.05 * (1 ... 5) * 40 * 0.1: of order one.
REST = dict(nx=64, ny=64, dt=0.1, nu=0.05, drag=0.02, mean=(0.3, -0.2), nsteps=40, every=8,
            modes=((1, 1), (0, 1), (2, 1), (2, 0)), pair=((1, 0), (0, 2)))

# Figures of the GPU run on the MI355X against the float64 oracle or the analytic value, and their bounds: 3-7x the worst measured figure,
# rounded (they move by about two with shape and seed).  The exponents' figure is |lambda_gpu - lambda_ref| nsteps dt, the error of the
# summed logs, so that it does not depend on the length of the run; the logs' is |log R_kk - its reference|.
MEASURED = {
    'gram': 1.63e-15,              # max |G - G_numpy| / max |G_numpy|, float64 sums of the same float32 spectra in another order
    # max |G - I| after orthonormalize_tangents, K = 4 random vectors, and after lyapunov_spectrum on the three runs of GPU test 8
    'ortho_random': {'random': 3.06e-08, 'forced': 3.76e-08, 'linear': 2.97e-08, 'stochastic': 3.96e-08},
    'ortho_near': 3.20e-08,        # the same on the nearly dependent set
    'span': 3.65e-08,              # max over k of |d_k - sum_l <q_l, d_k> q_l| / |d_k| in the energy norm (random set)
    'logs': {'random': 1.59e-08, 'near': 2.22e-08},      # max |log R_kk - oracle|, the oracle on the GPU's own float32 spectra
    'spectrum': {'forced': 1.06e-07, 'linear': 1.80e-07, 'stochastic': 1.19e-07},
    'rest': {'drag': 4.32e-07, 'beta': 3.36e-07},
    'rest_pair': {'drag': 4.80e-07, 'beta': 5.37e-07},
    'single': 6.10e-08,            # K = 1 against lyapunov_exponent, the same inputs
}
BOUND = {
    'gram': 8e-15,                 # 4.9x
    'ortho_random': 2e-7,          # 5.1x the worst (after the stochastic run)
    'ortho_near': 1.5e-7,          # 4.7x
    'span': 1.8e-7,                # 4.9x
    'logs': 1e-7,                  # 4.5x the worst (the nearly dependent set)
    'spectrum': 8e-7,              # 4.4x the worst (linear)
    'rest': 2e-6,                  # 4.6x the worst (drag)
    'rest_pair': 2.5e-6,           # 4.7x the worst (beta)
    'single': 3e-7,                # 4.9x
}
# The diagonal of the Gram matrix against diagnostics(...).energy has no figure: both kernels walk a grid in the same order and form
# wt (x x + y y) / |k|^2 from the same values, so the two float64 sums are the same bits, and the test asks for that.


def tangent_fields(c, K):
    """float32 [K, B, nx, ny]: the vorticity perturbations of a case; member 0 is pspec_tangent_cases.inputs(c)['dw']."""
    nx, ny, B, Lx, Ly, mean = c
    s = C.seed(c)
    return np.stack([O.band_ic(B, nx, ny, s + 4000 + 100 * k, Lx, Ly, 1.0)[0] for k in range(K)]).astype(np.float32)


def near_fields(c, K):
    """float32 [K, B, nx, ny]: the nearly dependent set d_k = d_0 + NEAR e_k (k >= 1) of tangent_fields' members."""
    e = tangent_fields(c, K).astype(np.float64)
    d = e[:1] + NEAR * NEAR_AMP * e
    d[0] = e[0]
    return d.astype(np.float32)


def spectra(S, fields):
    """complex128 rfft2 spectra of float32 fields, masked as init_tangents masks them."""
    return S.M * np.fft.rfft2(np.asarray(fields, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def oracle_spectrum(run, wrong=None, K=K_SPECTRUM, nsteps=NSTEPS, every=EVERY):
    """float64 [B, K]: the finite-time exponents of the float64 scheme for the run's inputs.  Computed once per (run, variant): do not modify."""
    kind, c = run
    d = TC.inputs(c)
    S = TC.scheme(kind, c, d['dt'])
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    starts = None
    if kind == 'stochastic':
        starts = LA.stochastic_starts(S, LAC.amplitudes(c), TC.SEED, w, mean, nsteps)[0]
    return LY.Lyapunov(S, wrong).exponents(w, mean, spectra(S, tangent_fields(c, K)), nsteps, every, starts)[0]


@functools.lru_cache(maxsize=None)
def oracle_logs(wrong=None, near=False, K=K_ORTHO):
    """float64 [B, K]: log diag R of the factorisation of the random (near: the nearly dependent) set at CASES[0]."""
    c = CASES[0]
    S = TC.scheme('forced', c, TC.inputs(c)['dt'])
    return LY.Lyapunov(S, wrong).qr(spectra(S, (near_fields if near else tangent_fields)(c, K)))[1]


def rest_fields(pair=False):
    """float32 [K, 1, nx, ny]: the single modes of REST (pair: A + B and A - B) as cosines of unit amplitude."""
    nx, ny = REST['nx'], REST['ny']
    x, y = np.meshgrid(TWO_PI * np.arange(nx) / nx, TWO_PI * np.arange(ny) / ny, indexing='ij')
    wave = lambda m: np.cos(m[0] * x + m[1] * y)
    if pair:
        a, b = (wave(m) for m in REST['pair'])
        f = [a + b, a - b]
    else:
        f = [wave(m) for m in REST['modes']]
    return np.stack(f)[:, None].astype(np.float32)


def rest_rates(modes, beta=False):
    """Re(lambda) of the modes on the base at rest: -(nu |k|^2 + drag); the beta term is imaginary and changes nothing."""
    return np.array([-(REST['nu'] * (m[0] ** 2 + m[1] ** 2) + REST['drag']) for m in modes])
