"""CPU checks of the restatement of K tangent pairs with a scalar and of their Lyapunov spectrum (tests/pspec_scalar_lyapunov_oracle.py): its
Gram matrix against a direct physical-space computation, its factorisation, the analytic spectrum on the base at rest at finite time, and the
mutation tests: every deliberately wrong variant lies at least 10x the GPU bound from the right answer on the very inputs of the GPU tests
(tests/pspec_scalar_lyapunov_cases.py) where it can show; where it cannot, the input where it does is named below."""
import numpy as np
import pytest

import pspec_scalar_lyapunov_cases as SC
import pspec_scalar_lyapunov_oracle as SLY
import pspec_scalar_tangent_cases as TC

C0 = SC.CASES[0]


def scheme(kind='buoyant'):
    return TC.scheme(kind, C0, TC.inputs(C0)['dt'])


@pytest.mark.parametrize('weight', [1.0, SC.WEIGHT])
def test_gram_is_the_physical_space_inner_product(weight):
    """1/2 <du_k . du_l> + weight 1/2 <dtheta_k' dtheta_l'>, grid means of band-limited fields, the means of dtheta taken out."""
    S = scheme()
    Dw, Dt = SC.spectra(S, SC.tangent_fields(C0, 3))
    G = SLY.ScalarLyapunov(S, weight).gram(Dw, Dt)
    zero = np.zeros((C0[2], 2))
    vel = [tuple(S.irfft2(h) for h in S.velocity_hat(d, zero)) for d in Dw]
    th = [S.irfft2(d) for d in Dt]
    th = [t - t.mean(axis=(-1, -2), keepdims=True) for t in th]
    ref = np.empty_like(G)
    for k in range(3):
        for l in range(3):
            ref[:, k, l] = 0.5 * (vel[k][0] * vel[l][0] + vel[k][1] * vel[l][1]).mean(axis=(-1, -2)) + weight * 0.5 * (th[k] * th[l]).mean(axis=(-1, -2))
    err = float(np.abs(G - ref).max() / np.abs(ref).max())
    print('gram against physical space, weight %g: %.2e' % (weight, err))
    assert err <= 1e-13, err
    assert float(np.abs(np.diagonal(G, axis1=1, axis2=2)).min()) > 0


@pytest.mark.parametrize('near', [False, True], ids=['random', 'near'])
@pytest.mark.parametrize('weight', [1.0, SC.WEIGHT])
def test_qr_reproduces_d_and_is_orthonormal(weight, near):
    S = scheme()
    K = SC.K_ORTHO
    L = SLY.ScalarLyapunov(S, weight)
    Dw, Dt = SC.spectra(S, (SC.near_fields if near else SC.tangent_fields)(C0, K))
    Qw, Qt, logs = L.qr(Dw, Dt)
    G = L.gram(Qw, Qt)
    ortho = float(np.abs(G - np.eye(K)).max())
    R = np.stack([np.stack([L.dot(Qw[l], Qt[l], Dw[k], Dt[k])[..., 0, 0] for k in range(K)], axis=-1) for l in range(K)], axis=-2)      # [B, l, k]
    scale = np.sqrt(np.diagonal(L.gram(Dw, Dt), axis1=1, axis2=2)).max()
    lower = float(np.abs(np.tril(R, -1)).max() / scale)
    back = 0.0
    for k in range(K):
        rw = Dw[k] - sum(R[:, l, k][:, None, None] * Qw[l] for l in range(K))
        rt = Dt[k] - sum(R[:, l, k][:, None, None] * Qt[l] for l in range(K))          # the (0, 0) entries included: they combine with the rest
        back = max(back, float(np.abs(rw).max() / np.abs(Dw[k]).max()), float(np.abs(rt).max() / np.abs(Dt[k]).max()))
    diag = float(np.abs(np.log(np.diagonal(R, axis1=1, axis2=2)) - logs).max())
    print('qr weight %g %s: |G - I| %.2e, below the diagonal %.2e, D - Q R %.2e, log diag %.2e' % (weight, 'near' if near else 'random', ortho, lower, back, diag))
    # the nearly dependent set has a condition number near 1e5 in D itself: Gram-Schmidt done twice keeps Q orthonormal to round-off times a few
    assert ortho <= 1e-12 and lower <= 1e-12 and back <= 1e-12 and diag <= (1e-7 if near else 1e-12), (ortho, lower, back, diag)


@pytest.mark.parametrize('weight', [1.0, SC.WEIGHT])
def test_the_spectrum_on_the_base_at_rest_is_analytic_at_finite_time(weight):
    """(lambda_+, lambda_+, lambda_-, lambda_-) for any scalar_weight (SC.rest_fields' note), to RK4's truncation: measured 4.66e-10
    (weight 1) and 4.66e-10 (weight 4) as max |lambda - analytic| nsteps dt over 200 steps of dt = 0.01."""
    lp, lm = SC.rest_rates()[:2]
    assert abs(lp - TC.EIGEN_EXPONENT) < 1e-9 and lm < -1.0
    lam = SC.oracle_rest(weight)
    err = float(np.abs(lam - np.array([lp, lp, lm, lm])).max() * SC.EIGEN['nsteps'] * SC.EIGEN['dt'])
    print('rest spectrum of the restatement, weight %g: %s, error x T %.2e' % (weight, lam, err))
    assert err <= 1e-8, err


# Where each wrong variant shows, on the GPU tests' own inputs: ('spectrum', kind, weight) is GPU test 11's run of that kind, ('logs', near,
# weight) GPU test 10's set.  normalise_only, no_scalar_in_product and mean_in_product show in both; first_pass_logs only on the nearly
# dependent set (the second pass's logs of a random set are under float32 round-off: pspec_lyapunov_cases' note); shared_accumulator only
# where members are stepped; weight_ignored only at a scalar_weight != 1, so at SC.WEIGHT, which both GPU tests also run.
SHOWS = {
    'normalise_only': [('spectrum', k, 1.0) for k in SC.SPECTRUM_KINDS] + [('logs', False, 1.0), ('logs', True, 1.0)],
    'no_scalar_in_product': [('spectrum', k, 1.0) for k in SC.SPECTRUM_KINDS] + [('logs', False, 1.0), ('logs', False, SC.WEIGHT)],
    'mean_in_product': [('spectrum', k, 1.0) for k in SC.SPECTRUM_KINDS] + [('logs', False, 1.0), ('logs', False, SC.WEIGHT)],
    'first_pass_logs': [('logs', True, 1.0), ('logs', True, SC.WEIGHT)],
    'shared_accumulator': [('spectrum', k, 1.0) for k in SC.SPECTRUM_KINDS],
    'weight_ignored': [('spectrum', 'buoyant', SC.WEIGHT), ('logs', False, SC.WEIGHT)],
}


def test_every_wrong_variant_is_listed():
    assert set(SHOWS) == set(SLY.WRONG)


@pytest.mark.parametrize('wrong', SLY.WRONG)
def test_the_gpu_bounds_catch_every_wrong_variant(wrong):
    for what, which, weight in SHOWS[wrong]:
        if what == 'spectrum':
            run = (which, C0)
            T = SC.NSTEPS * TC.inputs(C0)['dt']
            dist = float(np.abs(SC.oracle_spectrum(run, wrong, weight) - SC.oracle_spectrum(run, None, weight)).max() * T)
            bound = SC.BOUND['spectrum']
        else:
            dist = float(np.abs(SC.oracle_logs(wrong, which, weight) - SC.oracle_logs(None, which, weight)).max())
            bound = SC.BOUND['logs']
        print('%s at %s %s weight %g: %.2e = %.0fx the bound' % (wrong, what, which, weight, dist, dist / bound))
        assert dist >= 10 * bound, (wrong, what, which, weight, dist, bound)


def test_member_zero_is_the_single_tangents_pair():
    dw, dth = SC.tangent_fields(C0, 2)
    d = TC.inputs(C0)
    assert np.array_equal(dw[0], d['dw']) and np.array_equal(dth[0], d['dtheta'])
