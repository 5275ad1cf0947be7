"""Linear-operator cases of the periodic spectral solver: full-band inputs of tests/pspec_cases.py under the Kolmogorov force of
tests/pspec_forced_cases.py with hyperviscosity, hypofriction, the beta effect, a drag and the viscosity all acting
(tests/test_gpu_pspec_linear.py runs them on the GPU against tests/pspec_linear_oracle.py; tests/test_oracle_pspec_linear.py shows on the CPU
that their bounds would catch a beta of the wrong sign or on the wrong wavenumber, conjugated factors, a hyperviscosity of the wrong order, a
missing hypofriction and an E^2 rotated by the angle of E).

The parameters are dimensionless per step, so that every term matters in NSTEPS = 12 steps at any shape (dt = the CFL step of pspec_cases):
    hyperviscosity  nu_h = 5 / (dt K^2p), p = 4     K the kept band's corner wavenumber: the band edge is stiff (nu_h K^2p dt = 5), mid-band mild
    hypofriction    mu = 0.05 k1^2q / dt, q = 1     k1 = min(2 pi / Lx, 2 pi / Ly): 0.05 per step on the gravest mode
    beta            0.2 (2 pi / Lx) / dt            0.2 rad per step on the gravest x-mode
    drag 0.1, nu = pspec_cases.NU, Kolmogorov force (KF, AMP) of pspec_forced_cases
Bounds: the project's own, pspec_cases.BOUND_W, BOUND_UV, BOUND_P (buoyant pressure: pspec_buoyant_cases.BOUND_P).

Measured on the MI355X, rel-L2 against the float64 restatement, worst over the seven trajectory cases: what 2.72e-7 (64x1024; margin 7.3x),
u, v 4.87e-7 (64x1024; 4.1x), p 5.97e-6 (128x512; 17x), buoyant p 3.61e-7 (12x), that' 4.25e-7 (4.7x): no bound was changed.  Every figure,
the stiff step, the Rossby wave and the linear rates: MEASURED at the end of this file (profiles/pspec_linear_run.json).
"""
import numpy as np

import pspec_buoyant_cases as BC
import pspec_cases as C
import pspec_forced_cases as FC
import pspec_linear_oracle as LO
import pspec_oracle as O
import pspec_scalar_cases as SC
import pspec_stochastic_cases as XC
import pspec_stochastic_oracle as ST

TWO_PI = C.TWO_PI
NSTEPS = C.NSTEPS
P, Q, DRAG = 4, 1, 0.1
HYPER_PER_STEP, HYPO_PER_STEP, BETA_PER_STEP = 5.0, 0.05, 0.2

# the smallest shapes at which the table's indexing can go wrong: two column tiles with a ragged tail (3 * 22 = 66 columns in tiles of 64); the
# 1 x 4 box (anisotropic wavenumbers, many shells); the 4-line tiles of N = 1024; my1 = 342
CASES = [C.FULL_BAND[k] for k in (0, 1, 6, 7)]
assert [c[:3] for c in CASES] == [(64, 64, 3), (128, 512, 2), (1024, 64, 2), (64, 1024, 2)]
CASE_IDS = [C.case_id(c) for c in CASES]
SCALAR_CASE, BUOYANT_CASE = SC.CASES[0], BC.CASES[0]
assert SCALAR_CASE[:3] == (64, 64, 3) and BUOYANT_CASE[:3] == (64, 64, 3)
# the grid-stride loop: 400 * 22 = 8800 columns > 2048 workgroups x 4 lines at N = 1024
STRIDE_CASE = (1024, 64, 400, TWO_PI, TWO_PI, (0.0, 0.0))


def corner(nx, ny, Lx, Ly):
    """K: the wavenumber of the kept band's corner."""
    return float(np.hypot(TWO_PI / Lx * ((nx - 1) // 3), TWO_PI / Ly * (O.kept_y(ny) - 1)))


def params(nx, ny, Lx, Ly, dt, hyper_per_step=HYPER_PER_STEP):
    """dict(hyper=(nu_h, P), hypo=(mu, Q), beta=...) of a shape and step."""
    k1 = min(TWO_PI / Lx, TWO_PI / Ly)
    return dict(hyper=(hyper_per_step / (dt * corner(nx, ny, Lx, Ly) ** (2 * P)), P), hypo=(HYPO_PER_STEP * k1 ** (2 * Q) / dt, Q),
                beta=BETA_PER_STEP * (TWO_PI / Lx) / dt)


def scheme(nx, ny, dt, Lx, Ly, kind='flow', forced=True, drag=DRAG, **kw):
    """The restatement of a case.  kind 'flow': no scalar; 'scalar': kappa and G of pspec_scalar_cases; 'buoyant': plus b of pspec_buoyant_cases.
    kw overrides hyper, hypo, beta and passes mutate."""
    for k, v in params(nx, ny, Lx, Ly, dt).items():
        kw.setdefault(k, v)
    if kind != 'flow':
        kw.update(kappa=SC.KAPPA, grad=SC.GRAD)
    if kind == 'buoyant':
        kw['buoy'] = BC.BUOY
    S = LO.LinearScheme(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=drag, **kw)
    return S.kolmogorov_forcing(FC.KF, FC.AMP) if forced else S


def solver(case, dt, kind='flow', forced=True, stochastic=None, **kw):
    """The PeriodicSolver of a case (GPU tests), its parameters those of scheme(); stochastic = (rate, k_lo, k_hi) adds the ring force."""
    from nns.periodic import PeriodicSolver
    nx, ny, B, Lx, Ly, _ = case
    pr = params(nx, ny, Lx, Ly, dt)
    kw.setdefault('hyperviscosity', pr['hyper'])
    kw.setdefault('hypofriction', pr['hypo'])
    kw.setdefault('beta', pr['beta'])
    if kind != 'flow':
        kw.update(kappa=SC.KAPPA, scalar_gradient=SC.GRAD)
    if kind == 'buoyant':
        kw['buoyancy'] = BC.BUOY
    s = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=DRAG, **kw)
    if forced:
        s.kolmogorov_forcing(FC.KF, FC.AMP)
    if stochastic is not None:
        s.ring_forcing(stochastic[0], stochastic[1], stochastic[2], seed=XC.SEED)
    return s


_RUNS = {}


def reference(kind, case, **kw):
    """kind 'flow', 'scalar', 'buoyant', 'stochastic': (S, inputs, w, t or None, mean, extra) after NSTEPS steps of the restatement from the
    float32 full-band inputs; extra = (rate, amp) of the ring force of pspec_stochastic_cases (traj_ring, traj_rate) for 'stochastic', else None.
    Computed once per session, shared and read-only.  kw (mutations, switched-off terms) makes a separate entry."""
    key = (kind, case, tuple(sorted(kw.items())))
    if key not in _RUNS:
        nx, ny, B, Lx, Ly, _ = case
        u0, v0, dt = C.full_band_input(*case)
        S = scheme(nx, ny, dt, Lx, Ly, kind if kind != 'stochastic' else 'flow', **kw)
        w0, mean = S.init(u0, v0)
        th0 = SC.scalar_input(*case) if kind in ('scalar', 'buoyant') else None
        extra = None
        if kind == 'stochastic':
            rate = XC.traj_rate(S, w0)
            amp = ST.amplitude_table(nx, ny, Lx, Ly, ST.ring_rates(nx, ny, Lx, Ly, rate, *XC.traj_ring(nx, ny, Lx, Ly)))
            w, t, extra = ST.Stochastic(S, amp, XC.SEED).step(w0, mean, NSTEPS), None, (rate, amp)
        elif th0 is None:
            w, t = S.step(w0, mean, NSTEPS), None
        else:
            w, t = S.step(w0, S.init_scalar(th0), mean, NSTEPS)
        ins = (u0, v0) if th0 is None else (u0, v0, th0)
        for a in ins + (w, mean) + (() if t is None else (t,)):
            a.setflags(write=False)
        _RUNS[key] = (S, ins, w, t, mean, extra)
    return _RUNS[key]


def errors(S, w, mean, ref_w, ref_mean):
    """(rel-L2 of what, of u, of v, of p) of a state (w, mean) against the reference state, both in the restatement's layout."""
    from conftest import rel_l2
    got, ref = S.fields(w, mean), S.fields(ref_w, ref_mean)
    return (SC.rel_l2c(S.compact(w), S.compact(ref_w)),) + tuple(rel_l2(g, r) for g, r in zip(got, ref))


# ---- the analytic Rossby wave: (nx, ny, Lx, Ly, m, U, dt); 200 steps.  beta = 4: omega = -beta kx / |k|^2 = -8 / 13, so over t = 10 the phase turns
# by -omega t = 6.15 rad on top of the advection's k . U t = 4 rad; nu, drag, nu_h and mu together damp the amplitude to 0.879.
WAVE = (64, 64, TWO_PI, TWO_PI, (2, 3), (0.5, -0.2), 0.05)
WAVE_STEPS, WAVE_BETA, WAVE_NU, WAVE_DRAG, WAVE_HYPER, WAVE_HYPO = 200, 4.0, 5e-4, 3.65e-3, (2e-7, 3), (3e-2, 1)
# max error of the vorticity over the grid / its decayed amplitude: the bound of the buoyant plane waves of pspec_buoyant_cases.WAVES
# (tests/test_gpu_pspec_buoyant.py: WAVE_BOUND), the project's 200-step analytic bound
WAVE_BOUND = 2.3e-6


def wave_damping():
    """-Re(lambda) of the wave's mode."""
    nx, ny, Lx, Ly, m, U, dt = WAVE
    k2 = (TWO_PI * m[0] / Lx) ** 2 + (TWO_PI * m[1] / Ly) ** 2
    return WAVE_NU * k2 + WAVE_DRAG + WAVE_HYPER[0] * k2 ** WAVE_HYPER[1] + WAVE_HYPO[0] * k2 ** -WAVE_HYPO[1]


def wave_rk4_error(nsteps=WAVE_STEPS):
    """RK4's error after nsteps steps as a fraction of the amplitude, n (|k . U| dt)^5 / 120: only the advection by the mean flow is integrated
    by RK4 (it sits in N); the wave's own frequency and decay are in the Lawson factor, which is exact."""
    nx, ny, Lx, Ly, m, U, dt = WAVE
    return nsteps * (abs(TWO_PI * m[0] / Lx * U[0] + TWO_PI * m[1] / Ly * U[1]) * dt) ** 5 / 120


# ---- stiffness: one step with nu_h K^2p dt = 50 (the factor at the corner is exp(-50); an explicit RK4 would need nu_h K^2p dt < 2.8)
STIFF_PER_STEP = 50.0

MEASURED = """
rel-L2 against the float64 restatement after 12 steps, measured on the MI355X (profiles/pspec_linear_run.json); bounds 2e-6 (what, u, v),
1e-4 (p), 4.5e-6 (buoyant p):
  kind        shape       what      u         v         p         that'
  flow        64x64x3     2.55e-07  1.68e-07  2.23e-07  6.70e-07
  flow        128x512x2   2.48e-07  2.72e-07  3.06e-07  5.97e-06
  flow        1024x64x2   2.69e-07  2.45e-07  2.98e-07  1.24e-06
  flow        64x1024x2   2.72e-07  2.96e-07  4.87e-07  7.03e-07
  scalar      64x64x3     2.55e-07  1.68e-07  2.23e-07  6.70e-07  4.25e-07
  buoyant     64x64x3     2.40e-07  1.52e-07  2.01e-07  3.61e-07  2.62e-07
  stochastic  64x64x3     2.08e-07  1.58e-07  1.88e-07  4.80e-07
Margins: what 7.3x, u and v 4.1x, p 17x, buoyant p 12x: no bound was changed.
Stiff step (nu_h K^8 dt = 50), 64x64x3: what 1.45e-07, u 1.16e-07, v 1.38e-07, p 6.92e-07.
Rossby wave, 200 steps: max error / amplitude w 1.14e-06, u and v 2.68e-07 (bound 2.3e-6: 2.0x).
j = 0 line after 12 steps: Hermitian defect 1.8e-07 of its largest element (3 float32 ulp; bound 100 ulp).
linear_spectrum against the restatement of the same float32 state, 128x512 (240 shells): D_E 8.9e-16, D_Z 7.8e-16 relative per shell (bound 1e-11);
the total budget against power_in + sum_s D_E: 4.5e-08 of the transfer's scale (bound 2e-6); inactive against -2 nu Z - 2 drag E: 4.4e-16.
"""
