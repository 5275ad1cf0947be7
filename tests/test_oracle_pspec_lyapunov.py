"""CPU checks of the restatement (tests/pspec_lyapunov_oracle.py) that the GPU's K tangents and Lyapunov spectrum
(nns.periodic.PeriodicSolver.step_tangents / orthonormalize_tangents / lyapunov_spectrum) are compared against: its factorisation against
numpy.linalg.qr, the analytic exponents of a base at rest, the distance of every deliberately wrong spectrum from the right one on the
inputs of the GPU tests, and kaplan_yorke_dimension."""
import numpy as np
import pytest
import torch

import pspec_lyapunov_cases as LC
import pspec_lyapunov_oracle as LY
import pspec_tangent_cases as TC
import pspec_tangent_oracle as T


# ---------------------------------------------------------------------------------------------------- 1. the factorisation
@pytest.mark.parametrize('near', [False, True], ids=['random', 'near'])
def test_qr_against_numpy_qr_of_the_weight_scaled_real_vectors(near):
    c = TC.CASES[0]
    S = TC.scheme('forced', c, TC.inputs(c)['dt'])
    L = LY.Lyapunov(S)
    D = LC.spectra(S, (LC.near_fields if near else LC.tangent_fields)(c, LC.K_ORTHO))
    Q, logs = L.qr(D)
    assert np.abs(L.gram(Q) - np.eye(LC.K_ORTHO)).max() <= 1e-12
    sw = np.sqrt(L.weight())
    real = lambda Z, b: np.concatenate([(sw * Z[:, b].real).reshape(len(Z), -1), (sw * Z[:, b].imag).reshape(len(Z), -1)], axis=1).T
    for b in range(c[2]):
        q, r = np.linalg.qr(real(D, b))
        sign = np.sign(np.diagonal(r))
        assert np.abs(np.log(np.abs(np.diagonal(r))) - logs[b]).max() <= (1e-9 if near else 1e-12)
        assert np.abs(q * sign - real(Q, b)).max() <= (1e-6 if near else 1e-12)         # numpy's Householder loses cond(D) eps on the near set


# ---------------------------------------------------------------------------------------------------- 2. the base at rest
@pytest.mark.parametrize('beta', [0.0, 4.0], ids=['drag', 'beta'])
def test_the_oracle_gives_the_analytic_exponents_on_a_base_at_rest(beta):
    R = LC.REST
    S = T.TangentScheme(R['nx'], R['ny'], R['dt'], 1.0, R['nu'], drag=R['drag'], beta=beta)
    L = LY.Lyapunov(S)
    w = np.zeros((1, R['nx'], R['ny'] // 2 + 1), dtype=np.complex128)
    mean = np.array([R['mean']], dtype=np.float64)
    T_ = R['nsteps'] * R['dt']
    lam = L.exponents(w, mean, LC.spectra(S, LC.rest_fields()), R['nsteps'], R['every'])[0][0]
    # RK4 of the advection by the mean flow: |k . U| dt <= 0.1, an amplitude error of (0.1)^6 / 144 per step at the most
    assert np.abs(lam - LC.rest_rates(R['modes'])).max() * T_ <= 1e-7, lam
    lam2 = L.exponents(w, mean, LC.spectra(S, LC.rest_fields(pair=True)), R['nsteps'], R['every'])[0][0]
    assert abs(lam2.sum() - LC.rest_rates(R['pair']).sum()) * T_ <= 1e-7, lam2
    assert abs(lam2[0] - lam2[1]) * T_ > 1e-2                      # the two exponents themselves are not the modes' rates: only their sum is


# ---------------------------------------------------------------------------------------------------- 3. the wrong variants
def distances(wrong):
    """The distance of a wrong variant from the right oracle in the figure of each GPU check that could see it, on that check's own
    inputs, over the check's bound: (spectrum runs, logs of the random set, logs of the nearly dependent set)."""
    T_ = LC.NSTEPS * TC.inputs(TC.CASES[0])['dt']
    spec = max(float(np.abs(LC.oracle_spectrum(run, wrong) - LC.oracle_spectrum(run)).max() * T_) for run in LC.SPECTRUM_RUNS)
    logs = [float(np.abs(LC.oracle_logs(wrong, near) - LC.oracle_logs(None, near)).max()) for near in (False, True)]
    return spec / LC.BOUND['spectrum'], logs[0] / LC.BOUND['logs'], logs[1] / LC.BOUND['logs']


@pytest.mark.parametrize('wrong', LY.WRONG)
def test_every_wrong_variant_is_ten_bounds_away_on_the_gpu_tests_inputs(wrong):
    """normalise_only, enstrophy_product, no_initial_orthonormalisation and shared_accumulator change the exponents of GPU test 8 on each of
    its runs; first_pass_logs changes nothing there that float32 could see (the Gram matrix of well-separated vectors is factored to
    float64 round-off in one pass) and is caught by the logs of the nearly dependent set of GPU test 7."""
    spec, logs, near = distances(wrong)
    print('%s: distance / bound: spectrum %.3g, logs (random) %.3g, logs (near) %.3g' % (wrong, spec, logs, near))
    assert max(spec, logs, near) >= 10.0
    if wrong != 'first_pass_logs':
        T_ = LC.NSTEPS * TC.inputs(TC.CASES[0])['dt']
        for run in LC.SPECTRUM_RUNS:
            assert np.abs(LC.oracle_spectrum(run, wrong) - LC.oracle_spectrum(run)).max() * T_ >= 10 * LC.BOUND['spectrum'], run


def test_the_bounds_are_three_to_seven_times_the_worst_measured_figure():
    for key, bound in LC.BOUND.items():
        m = LC.MEASURED[key]
        worst = max(m.values()) if isinstance(m, dict) else m
        assert 3.0 <= bound / worst <= 7.0, (key, bound, worst)


# ---------------------------------------------------------------------------------------------------- 4. the Kaplan-Yorke dimension
def test_kaplan_yorke_dimension():
    from nns.periodic import kaplan_yorke_dimension
    spectra = [[0.9, 0.0, -14.57],            # Lorenz 63: 2 + 0.9 / 14.57
               [-14.57, 0.9, 0.0],            # the same, unsorted
               [-0.1, -0.2, -0.3],            # lambda_1 < 0: 0
               [0.5, 0.2, -0.1],              # every partial sum >= 0: K, a lower bound
               [0.3, -0.3, -1.0],             # S_2 = 0 exactly: 2
               [1.0, -4.0, -5.0]]             # 1 + 1 / 4
    want = [2 + 0.9 / 14.57, 2 + 0.9 / 14.57, 0.0, 3.0, 2.0, 1.25]
    got = kaplan_yorke_dimension(torch.tensor(spectra, dtype=torch.float64))
    assert got.dtype == torch.float64 and tuple(got.shape) == (6,)
    assert np.abs(got.numpy() - np.array(want)).max() <= 1e-15
    assert np.abs(np.array([LY.kaplan_yorke(s) for s in spectra]) - np.array(want)).max() <= 1e-15
    batched = kaplan_yorke_dimension(torch.tensor([spectra, spectra], dtype=torch.float64))
    assert tuple(batched.shape) == (2, 6) and torch.equal(batched[1], got)
    assert torch.isnan(kaplan_yorke_dimension(torch.tensor([0.1, float('nan'), -1.0], dtype=torch.float64)))
    assert float(kaplan_yorke_dimension(torch.tensor([0.25], dtype=torch.float64))) == 1.0
