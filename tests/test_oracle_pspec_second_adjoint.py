"""CPU checks of the float64 restatement of the second-order adjoint (tests/pspec_second_adjoint_oracle.py): against central differences of
the reverse-mode restatement it differentiates, the symmetry of the Hessian it stands for, its first-order results against the parents' to
the last bit, and the distance of every deliberately wrong scheme from it on the GPU test's own inputs, measured against that test's bound
(tests/pspec_second_adjoint_cases.py).  No GPU."""
import inspect

import numpy as np
import pytest

import pspec_linear_adjoint_oracle as LA
import pspec_linear_cases as LC
import pspec_oracle as O
import pspec_second_adjoint_cases as SC
import pspec_second_adjoint_oracle as S2
import pspec_tangent_oracle as T

FD_BOUND = 1e-8            # central differences of step_vjp, step 1e-5 in float64: truncation ~ 1e-10 |d^3|, rounding ~ 1e-16 / 1e-5 (5.6e-12 measured)
SYMMETRY_BOUND = 1e-12     # two float64 evaluations of one bilinear form (2e-16 measured)


def build(nx, ny, B, linear, seed=11):
    """(S, w, mean, dw, dg, lam, dlam) of a small problem: a mean flow, a per-grid source, real or complex E."""
    Lx, Ly = 2 * np.pi, 2 * np.pi
    u0, v0 = O.band_ic(B, nx, ny, seed, Lx, Ly, 1.0, mean=(0.3, -0.2))
    dt = O.cfl_dt(nx, ny, Lx, Ly, 1.5)
    kw = LC.params(nx, ny, Lx, Ly, dt) if linear else {}
    S = S2.SecondAdjointScheme(nx, ny, dt, SC.RHO, SC.NU, Lx, Ly, drag=SC.DRAG, **kw)
    S.set_forcing(*O.band_ic(B, nx, ny, seed + 1, Lx, Ly, SC.TC.FORCE))
    w, mean = S.init(u0, v0)
    draw = lambda k, amp=1.0: S.M * np.fft.rfft2(O.band_ic(B, nx, ny, seed + k, Lx, Ly, amp)[0])
    return S, w, mean, draw(2), draw(3, SC.TC.FORCE), draw(4), draw(5)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize('nsteps', [1, 3])
@pytest.mark.parametrize('linear', [False, True], ids=['real-E', 'complex-E'])
@pytest.mark.parametrize('shape', [(64, 64), (64, 128)], ids=['64x64', '64x128'])
def test_against_central_differences_of_the_reverse_mode(shape, linear, nsteps):
    S, w, mean, dw, dg, lam, dlam = build(shape[0], shape[1], 2, linear)
    out = S.step_second_vjp(w, mean, dw, dg, lam, dlam, nsteps)
    g0, e = S.g, 1e-5

    def vjp(sign):
        S.g = g0 + sign * e * dg
        try:
            return S.step_vjp(w + sign * e * dw, mean, lam + sign * e * dlam, nsteps)
        finally:
            S.g = g0
    (wp, gp), (wm, gm) = vjp(1.0), vjp(-1.0)
    errs = rel((wp - wm) / (2 * e), out[2]), rel((gp - gm) / (2 * e), out[3])
    print('central differences %s %s %d steps: dwbar %.2e dgbar %.2e' % (shape, 'complex' if linear else 'real', nsteps, errs[0], errs[1]))
    assert max(errs) <= FD_BOUND, errs
    assert float(np.abs(out[2]).max()) > 0 and float(np.abs(out[3]).max()) > 0


@pytest.mark.parametrize('linear', [False, True], ids=['real-E', 'complex-E'])
def test_first_order_results_are_the_parents_bits(linear):
    S, w, mean, dw, dg, lam, dlam = build(64, 64, 2, linear)
    out = S.step_second_vjp(w, mean, dw, dg, lam, dlam, 3)
    kw = LC.params(64, 64, S.Lx, S.Ly, S.dt) if linear else {}
    A = LA.LinearAdjointScheme(64, 64, S.dt, SC.RHO, SC.NU, S.Lx, S.Ly, drag=SC.DRAG, **kw)
    J = T.TangentScheme(64, 64, S.dt, SC.RHO, SC.NU, S.Lx, S.Ly, drag=SC.DRAG, **kw)
    A.g = J.g = S.g
    wbar, gbar = A.step_vjp(w, mean, lam, 3)
    assert np.array_equal(out[0], wbar) and np.array_equal(out[1], gbar)
    assert np.array_equal(out[4], J.step_jvp(w, mean, dw, 3, dg=dg))
    # the direction does not touch them, and a zero direction gives a zero derivative
    zero = S.step_second_vjp(w, mean, 0 * dw, None, lam, None, 3)
    assert np.array_equal(zero[0], wbar) and np.array_equal(zero[1], gbar)
    assert float(np.abs(zero[2]).max()) == 0.0 and float(np.abs(zero[3]).max()) == 0.0 and float(np.abs(zero[4]).max()) == 0.0


@pytest.mark.parametrize('linear', [False, True], ids=['real-E', 'complex-E'])
def test_the_hessian_of_a_least_squares_loss_is_symmetric(linear):
    """l = 1/2 sum (w_N - obs)^2: lam = w_N - obs, dlam = dw_N; <a, H b> = <b, H a> jointly in (w, g)."""
    S, w, mean, aw, ag, obs, bw = build(64, 64, 2, linear)
    bg = S.M * np.fft.rfft2(O.band_ic(2, 64, 64, 99, S.Lx, S.Ly, SC.TC.FORCE)[0])
    lam = S.step(w, mean, 3) - obs

    def H(dw, dg):
        dlam = S.step_second_vjp(w, mean, dw, dg, lam, None, 3)[4]
        out = S.step_second_vjp(w, mean, dw, dg, lam, dlam, 3)
        return out[2], out[3]
    Ha, Hb = H(aw, ag), H(bw, bg)
    lhs = S.pair(aw, Hb[0]).sum() + S.pair(ag, Hb[1]).sum()
    rhs = S.pair(bw, Ha[0]).sum() + S.pair(bg, Ha[1]).sum()
    scale = np.sqrt(S.pair(aw, aw).sum() + S.pair(ag, ag).sum()) * np.sqrt(S.pair(Hb[0], Hb[0]).sum() + S.pair(Hb[1], Hb[1]).sum())
    err = abs(lhs - rhs) / scale
    print('symmetry %s: <a, H b> %.15e <b, H a> %.15e scaled difference %.2e' % ('complex' if linear else 'real', lhs, rhs, err))
    assert err <= SYMMETRY_BOUND, err
    # the part a Gauss-Newton product drops is a real share of it
    gn = S.step_second_vjp(w, mean, aw, ag, 0 * lam, S.step_second_vjp(w, mean, aw, ag, lam, None, 3)[4], 3)
    share = rel(gn[2], Ha[0])
    print('the share of H a that Gauss-Newton drops: %.2f' % share)
    assert share > 0.05


def distance(run, setting, wrong):
    ref, got = SC.oracle_second(run, setting, None, 'grid'), SC.oracle_second(run, setting, wrong, 'grid')
    return max(SC.rel(got[2], ref[2]), SC.rel(got[3], ref[3]))


@pytest.mark.parametrize('setting', SC.SETTINGS)
@pytest.mark.parametrize('run', SC.RUNS, ids=SC.run_id)
def test_every_wrong_scheme_is_far_beyond_the_gpu_bound(run, setting):
    shown = [w for w in S2.WRONG if SC.wrong_shows(run, setting, w)]
    assert 'gauss_newton' in shown and 'no_ilap_d' in shown
    for wrong in shown:
        d = distance(run, setting, wrong)
        print('%s %s %s: %.2e = %.0fx the bound' % (SC.run_id(run), setting, wrong, d, d / SC.BOUND[setting]))
        assert d >= 10 * SC.BOUND[setting], (wrong, d)


def test_every_wrong_scheme_shows_somewhere_in_both_settings_or_in_the_pure_one():
    for wrong in S2.WRONG:
        for setting in SC.SETTINGS:
            where = [r for r in SC.RUNS if SC.wrong_shows(r, setting, wrong)]
            assert where, (wrong, setting)
    # what cannot show does not: without a mean flow mean_in_du is the right scheme, with a real E so is not_conjugated
    assert distance(SC.RUNS[3], 'pure', 'mean_in_du') < 1e-8
    assert distance(SC.RUNS[0], 'pure', 'not_conjugated') == 0.0
    with pytest.raises(ValueError):
        S2.SecondAdjointScheme(64, 64, 0.01, 1.0, 1e-3, wrong='no_such_scheme')


def test_the_bounds_follow_the_measurements():
    assert set(SC.MEASURED) == {(SC.run_id(r), s) for r in SC.RUNS for s in SC.SETTINGS}
    for setting in SC.SETTINGS:
        worst = max(max(v) for k, v in SC.MEASURED.items() if k[1] == setting)
        assert 3 * worst <= SC.BOUND[setting] <= 7 * worst, (setting, worst)
        assert SC.BOUND[setting] < 1e-5
    assert set(SC.SYM_MEASURED) == set(SC.KINDS)
    assert 3 * max(SC.SYM_MEASURED.values()) <= SC.SYM_BOUND <= 7 * max(SC.SYM_MEASURED.values())


def test_entry_point_signatures():
    from nns import ops
    from nns.periodic import PeriodicSolver, SecondOrderRun, SecondOrderGradients
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(PeriodicSolver.second_order_forward) == ['self', 'w', 'dw', 'nsteps', 'mean', 'forcing', 'dforcing', 'clock', 'noise_ids']
    assert names(PeriodicSolver.hessian_vector_product) == ['self', 'loss', 'w', 'dw', 'nsteps', 'mean', 'forcing', 'dforcing', 'clock', 'noise_ids']
    assert names(SecondOrderRun.backward) == ['self', 'lam', 'dlam']
    assert SecondOrderGradients._fields == ('wbar', 'dwbar', 'gbar', 'dgbar')
    assert names(ops.spec_ns_second_adjoint_workspace) == ['B', 'nx', 'ny']
    assert names(ops.spec_ns_second_adjoint_) == ['what0', 'dwhat0', 'mean', 'ghat', 'dghat', 'lam', 'dlam', 'gbar', 'dgbar', 'work', 'ny', 'Lx', 'Ly',
                                                  'dt', 'nu', 'drag', 'lin']
    assert names(S2.SecondAdjointScheme.step_second_vjp) == ['self', 'w', 'mean', 'dw', 'dg', 'lam', 'dlam', 'nsteps', 'starts']
    doc = PeriodicSolver.__doc__
    assert 'hessian_vector_product' in doc and 'reverse mode through the tangent (Hessian-vector products)' not in doc
