"""CPU checks of the restatement tests/pspec_linear_oracle.py alone (no GPU, no library): that the bounds of tests/pspec_linear_cases.py would
catch each wrong scheme and each term switched off, the analytic Rossby wave, that with every new parameter zero the scheme is the parents' bit
for bit, that the per-shell budget with D_E closes against a central difference of the energy, and that beta does not enter D_E."""
import numpy as np
import pytest

import pspec_buoyant_cases as BC
import pspec_cases as C
import pspec_forced_cases as FC
import pspec_forced_oracle as F
import pspec_linear_cases as LC
import pspec_linear_oracle as LO
import pspec_scalar_cases as SC
import pspec_spectrum_oracle as PO

OFF = [('no hyperviscosity', dict(hyper=(0.0, LC.P))), ('no hypofriction', dict(hypo=(0.0, LC.Q))), ('no beta', dict(beta=0.0)),
       ('no drag', dict(drag=0.0))]
WRONG = [(m, dict(mutate=m)) for m in LO.MUTATIONS] + OFF


@pytest.mark.parametrize('case', LC.CASES[:2], ids=LC.CASE_IDS[:2])
def test_every_mutation_and_every_missing_term_misses_the_bounds(case):
    # (64, 64, 3) and (128, 512, 2) on the 1 x 4 box: each wrong scheme moves what, (u, v) and p by more than 10 x the bounds the GPU run is held
    # to (the least: the drag of 0.1 over the 12 short steps of 128 x 512, 23 x BOUND_P; every mutation of the new terms >= 300 x)
    S, ins, w, t, mean, _ = LC.reference('flow', case)
    E0, E1 = S.diag(S.init(*ins)[0])[0], S.diag(w)[0]
    print('%s: energy after %d steps / at the start: %s' % (C.case_id(case), LC.NSTEPS, ['%.3f' % r for r in E1 / E0]))
    assert np.all(E1 < 0.95 * E0) and np.all(np.isfinite(E1))
    worst = [np.inf, np.inf, np.inf]
    for name, kw in WRONG:
        Sm, _, wm, _, _, _ = LC.reference('flow', case, **kw)
        ew, eu, ev, ep = LC.errors(S, wm, mean, w, mean)
        print('  %-18s rel-L2 what %.2e  u %.2e  v %.2e  p %.2e' % (name, ew, eu, ev, ep))
        assert ew > 10 * C.BOUND_W and min(eu, ev) > 10 * C.BOUND_UV and ep > 10 * C.BOUND_P, (name, ew, eu, ev, ep)
        worst = [min(a, b) for a, b in zip(worst, (ew, min(eu, ev), ep))]
    print('  least: what %.2e (%.0f x bound), u / v %.2e (%.0f x), p %.2e (%.0f x)'
          % (worst[0], worst[0] / C.BOUND_W, worst[1], worst[1] / C.BOUND_UV, worst[2], worst[2] / C.BOUND_P))


def test_the_j0_line_stays_hermitian_and_the_operator_has_its_symmetry():
    case = LC.CASES[0]
    S, ins, w, t, mean, _ = LC.reference('flow', case)
    nx = S.nx
    line = w[..., 0]                                                               # [B, nx]: m_y = 0, both signs of m_x stored
    defect = np.abs(line[:, 1:nx // 2] - np.conj(line[:, :nx // 2:-1])).max() / np.abs(line).max()
    print('j = 0 line after %d steps: Hermitian defect %.1e of its largest element' % (LC.NSTEPS, defect))
    assert defect <= 1e-13
    lam = S.linear_operator()
    neg = (-np.arange(nx)) % nx
    assert np.array_equal(lam[neg, 0], np.conj(lam[:, 0]))                         # Re even, Im odd in k
    assert lam[0, 0] == 0 and np.all(lam.real[S.M > 0] < 0) and np.all(lam[S.M == 0] == 0)
    assert np.abs(lam.imag).max() > 0


def test_rossby_wave_with_mean_flow_200_steps():
    nx, ny, Lx, Ly, m, U, dt = LC.WAVE
    S = LO.LinearScheme(nx, ny, dt, C.RHO, LC.WAVE_NU, Lx, Ly, drag=LC.WAVE_DRAG, hyper=LC.WAVE_HYPER, hypo=LC.WAVE_HYPO, beta=LC.WAVE_BETA)
    u0, v0 = LO.rossby_wave(nx, ny, 0.0, m, LC.WAVE_BETA, LC.wave_damping(), U, Lx, Ly)[:2]
    w, mean = S.init(u0, v0)
    w = S.step(w, mean, LC.WAVE_STEPS)
    T = LC.WAVE_STEPS * dt
    ru, rv, rw, A, om = LO.rossby_wave(nx, ny, T, m, LC.WAVE_BETA, LC.wave_damping(), U, Lx, Ly)
    u, v, p = S.fields(w, mean)
    ew = np.abs(S.irfft2(w) - rw).max() / A
    eu = max(np.abs(u - ru).max(), np.abs(v - rv).max()) / A
    print('Rossby wave m %s on U %s, %d steps: omega t = %.3f rad, amplitude %.4f; max error / amplitude: w %.2e, u and v %.2e; RK4 estimate %.1e'
          % (m, U, LC.WAVE_STEPS, om * T, A, ew, eu, LC.wave_rk4_error()))
    assert abs(om * T) > 3 and abs(A - 0.879) < 1e-3
    # only the advection by the mean flow is RK4's; the wave's frequency and decay are exact in the factor
    assert max(ew, eu) <= 2 * LC.wave_rk4_error() + 1e-13
    assert np.abs(p).max() <= 1e-13
    # the wave does move westward: without beta the phase differs by omega t
    w0 = LO.LinearScheme(nx, ny, dt, C.RHO, LC.WAVE_NU, Lx, Ly, drag=LC.WAVE_DRAG, hyper=LC.WAVE_HYPER, hypo=LC.WAVE_HYPO).step(S.init(u0, v0)[0], mean, LC.WAVE_STEPS)
    i, j = m[0] % nx, m[1]
    assert abs(np.angle(w[i, j] / w0[i, j]) - (-om * T + 2 * np.pi)) < 1e-9 or abs(np.angle(w[i, j] / w0[i, j]) - (-om * T)) < 1e-9 \
        or abs(np.angle(w[i, j] / w0[i, j]) - (-om * T - 2 * np.pi)) < 1e-9


def test_with_every_new_parameter_zero_the_scheme_is_the_parents_bit_for_bit():
    case = LC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    u0, v0, dt = C.full_band_input(*case)
    th0 = SC.scalar_input(*case)
    zero = dict(hyper=(0.0, 4), hypo=(0.0, 1), beta=0.0)
    L = LO.LinearScheme(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG, **zero).kolmogorov_forcing(FC.KF, FC.AMP)
    P = F.ForcedScheme(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG).kolmogorov_forcing(FC.KF, FC.AMP)
    w, mean = P.init(u0, v0)
    assert np.array_equal(L.step(w, mean, 3), P.step(w, mean, 3))
    assert np.array_equal(L.step(w, mean, nsteps=2), P.step(w, mean, 2))
    Lb = LC.scheme(nx, ny, dt, Lx, Ly, 'buoyant', drag=FC.DRAG, **zero)
    Pb = BC.scheme(nx, ny, dt, Lx, Ly)
    t = Pb.init_scalar(th0)
    (a, at), (b, bt) = Lb.step(w, t, mean, 3), Pb.step(w, t, mean, 3)
    assert np.array_equal(a, b) and np.array_equal(at, bt)
    # and the full parameters change both
    Lf = LC.scheme(nx, ny, dt, Lx, Ly, 'buoyant', drag=FC.DRAG)
    assert not np.array_equal(Lf.step(w, t, mean, 3)[0], b)


def test_budget_with_the_linear_rates_closes_against_a_central_difference():
    # dE/dt = sum_s (T_E + F + D_E) at the state w against (E(+h) - E(-h)) / 2h, h = dt / 10, the two states one step of +-h away.
    # Tolerance: the central difference's own error h^2 |E'''| / 6 (the scheme's O(h^4) is far below), E''' from the second difference of
    # the budget's right-hand side over the same three states (itself good to O(h^2)), times 2 for the terms beyond, plus 1e-12 |dE/dt| for
    # rounding.  The stiff band edge (nu_h K^8 h = 0.5) makes E''' large, so this is a real constraint on h and is not a loose bound.
    case = LC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    S, ins, w, t, mean, _ = LC.reference('flow', case)
    h = S.dt / 10
    kw = dict(LC.params(nx, ny, Lx, Ly, S.dt))
    Sp, Sm = (LC.scheme(nx, ny, s * h, Lx, Ly, **kw) for s in (1, -1))
    wp, wm = Sp.step(w, mean, 1), Sm.step(w, mean, 1)
    cd = (S.diag(wp)[0] - S.diag(wm)[0]) / (2 * h)
    rhs = [S.energy_budget(x).sum(axis=-1) for x in (wm, w, wp)]
    e3 = np.abs(rhs[2] - 2 * rhs[1] + rhs[0]) / h ** 2
    tol = 2 * h ** 2 * e3 / 6 + 1e-12 * np.abs(rhs[1])
    print('budget closure: dE/dt %s, central difference off by %s, tolerance %s' % (rhs[1], np.abs(cd - rhs[1]), tol))
    assert np.all(np.abs(cd - rhs[1]) <= tol)
    assert np.all(tol <= 2e-4 * np.abs(rhs[1]))                                    # the check is sharp: 1e-4 of the rate itself
    # the pieces: D_E sums to the linear rate of the total energy, computed directly
    DE, DZ = S.linear_spectrum(w)
    wt = np.where(np.arange(ny // 2 + 1) == 0, 1.0, 2.0)[None, :]
    a2 = wt * (w.real ** 2 + w.imag ** 2) * S.linear_operator().real / float(nx * ny) ** 2
    assert np.allclose(DE.sum(axis=-1), (a2 * S.ik2).sum(axis=(-2, -1)), rtol=1e-12, atol=0)
    assert np.allclose(DZ.sum(axis=-1), a2.sum(axis=(-2, -1)), rtol=1e-12, atol=0)
    # a wrong D_E (the hyperviscosity of order p - 1) does not close
    bad = LC.scheme(nx, ny, S.dt, Lx, Ly, mutate='order').energy_budget(w).sum(axis=-1)
    assert np.all(np.abs(cd - bad) > 100 * tol)


def test_the_linear_rates_do_not_depend_on_beta_and_reduce_to_the_parents():
    case = LC.CASES[1]
    nx, ny, B, Lx, Ly, _ = case
    S, ins, w, t, mean, _ = LC.reference('flow', case)
    S0 = LC.scheme(nx, ny, S.dt, Lx, Ly, beta=0.0)
    for a, b in zip(S.linear_spectrum(w), S0.linear_spectrum(w)):
        assert np.array_equal(a, b) and np.all(a <= 0) and a.shape == (B, PO.shells(nx, ny, Lx, Ly)[2])
    plain = LC.scheme(nx, ny, S.dt, Lx, Ly, hyper=(0.0, 4), hypo=(0.0, 1), beta=0.0)
    sp = PO.spectrum(plain, w)
    DE, DZ = plain.linear_spectrum(w)
    ref = -2 * C.NU * sp['Z'] - 2 * LC.DRAG * sp['E']
    assert np.allclose(DE, ref, rtol=1e-12, atol=1e-15 * np.abs(ref).max())
    rhs, scale = PO.energy_budget(plain, w)
    assert np.allclose(plain.energy_budget(w), rhs, rtol=0, atol=1e-13 * scale.max())
