"""CPU checks of the restatement of the stochastic forcing (tests/pspec_stochastic_oracle.py) and of the host side of
nns.periodic.PeriodicSolver.set_stochastic_forcing / ring_forcing / stochastic_injection (the table is built without a GPU): Philox4x32-10
reproduces the Random123 known answers, the samples of the GPU cases have the moments of a complex standard normal, the table injects the rate
it is built for, the energy grows from rest at that rate, and the bounds of tests/test_gpu_pspec_stochastic.py would catch each mutation."""
import numpy as np
import pytest

import pspec_cases as C
import pspec_stochastic_cases as XC
import pspec_stochastic_oracle as ST
from pspec_scalar_cases import rel_l2c


# ---------------------------------------------------------------------------------------------------- 1. the generator
@pytest.mark.parametrize('counter, key, out', [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
], ids=['zeros', 'ones', 'pi'])
def test_philox_known_answers(counter, key, out):
    assert [int(v) for v in ST.philox4x32_10(counter, key)] == out
    # vectorised over leading axes, the same numbers
    both = ST.philox4x32_10(np.array([counter, [0, 0, 0, 0]]), np.array(key))
    assert [int(v) for v in both[0]] == out


def test_uniform_and_normal_maps():
    x = np.array([[0, 0, 7, 7], [0xffffffff, 0xffffffff, 7, 7], [0x80000000, 0x40000000, 7, 7]], dtype=np.uint32)
    u1, u2 = ST.uniforms(x)
    assert list(u1) == [2.0 ** -24, 1.0, 0.5 + 2.0 ** -24] and list(u2) == [0.0, 1.0 - 2.0 ** -24, 0.25]
    xi = ST.normals(x)
    assert xi[1] == 0.0                                                     # u1 = 1: the radius is sqrt(-ln 1) = 0
    assert abs(xi[0] - np.sqrt(24 * np.log(2.0))) < 1e-15                   # the largest radius, 4.08, at angle 0
    assert abs(xi[2] - 1j * np.sqrt(-np.log(0.5 + 2.0 ** -24))) < 1e-15     # a quarter turn


# ---------------------------------------------------------------------------------------------------- 2. moments of the GPU cases' samples
# deterministic given XC.SEED: (mean |xi|^2 - 1, |mean xi|) of the M = B x (forced stored modes) samples of step 0, bound 5 / sqrt(M)
RECORDED = {
    '64x64-B3': (1008, -1.293e-2, 4.374e-2), '1024x64-B2': (15012, -3.926e-4, 3.704e-3), '64x1024-B2': (14672, 3.329e-3, 7.923e-3),
    '128x512-B2': (11378, 1.648e-2, 3.376e-3), '1024x64-B400': (354400, -1.335e-3, 1.120e-3),
}


@pytest.mark.parametrize('case', XC.KICKS, ids=XC.KICK_IDS)
def test_moments_of_the_samples_of_the_gpu_cases(case):
    mask, xi = XC.kick_samples(case)
    m2, m1, bound = XC.moments(xi)
    print('%s: M = %d samples, mean |xi|^2 - 1 = %.3e, |mean xi| = %.3e, bound %.3e; max |xi| %.3f' % (XC.KICK_IDS[XC.KICKS.index(case)], xi.size,
                                                                                                  m2, m1, bound, np.abs(xi).max()))
    assert abs(m2) <= bound and m1 <= bound
    M, r2, r1 = RECORDED[XC.KICK_IDS[XC.KICKS.index(case)]]
    assert xi.size == M and abs(m2 - r2) <= 1e-3 * abs(r2) + 1e-6 and abs(m1 - r1) <= 1e-3 * r1 + 1e-6
    assert np.abs(xi).max() <= np.sqrt(24 * np.log(2.0))
    # the ring leaves modes inside and outside it and, unless it lies beyond the x band (64 x 1024), reaches the j = 0 line's mirror half, where
    # the conjugation acts
    nx = case[0]
    assert 0 < mask.sum() < mask.size and np.array_equal(mask[0, 1:nx // 2], mask[0, :nx // 2:-1])
    assert mask[0, nx // 2:].any() == (XC.kick_ring(*case)[0] <= C.TWO_PI / case[3] * ((nx - 1) // 3))
    assert mask[0, nx // 2:].any() or case[:2] == (64, 1024)


def test_samples_are_independent_over_steps_ids_and_modes_and_hermitian_on_the_j0_line():
    nx, ny = 64, 64
    a = ST.xi_stored(nx, ny, XC.SEED, 0, [0, 1, 0])
    b = ST.xi_stored(nx, ny, XC.SEED, 1, [0, 1, 0])
    assert np.array_equal(a[0], a[2]) and not np.any(a[0] == a[1]) and not np.any(a[0] == b[0])
    assert not np.any(ST.xi_stored(nx, ny, XC.SEED + 1, 0, [0])[0] == a[0]) and not np.any(ST.xi_stored(nx, ny, XC.SEED + 2 ** 32, 0, [0])[0] == a[0])
    assert np.array_equal(a[0, 0, 1:nx // 2], np.conj(a[0, 0, :nx // 2:-1]))
    assert len(np.unique(a[0, 1:])) == a[0, 1:].size                       # no two modes share a sample off the j = 0 line
    assert np.array_equal(ST.xi_stored(nx, ny, XC.SEED, 2 ** 32 + 5, [3])[0] == ST.xi_stored(nx, ny, XC.SEED, 5, [3])[0], np.zeros((22, 64), bool))


# ---------------------------------------------------------------------------------------------------- 3. the table and its injection
@pytest.mark.parametrize('box', [(64, 64, C.TWO_PI, C.TWO_PI, 4.0, 6.0), (128, 512, 1.0, 4.0, 25.0, 38.0), (1024, 64, C.TWO_PI, C.TWO_PI, 85.0, 256.0)],
                         ids=['64x64', '128x512', '1024x64'])
def test_solver_table_is_the_oracles_and_injects_the_rate(box):
    from nns.periodic import PeriodicSolver
    nx, ny, Lx, Ly, k_lo, k_hi = box
    rate = 0.37
    s = PeriodicSolver(nx, ny, 0.01, 1.0, 0.0, Lx=Lx, Ly=Ly)
    assert s.stoch_amp is None and not s.stochastic_injection().any()
    assert s.ring_forcing(rate, k_lo, k_hi, seed=XC.SEED) is s and s.stoch_seed == XC.SEED
    k, dk = s.shells()
    ref = ST.amplitude_table(nx, ny, Lx, Ly, ST.ring_rates(nx, ny, Lx, Ly, rate, k_lo, k_hi))
    assert s.stoch_amp.dtype == np.float32 and s.stoch_amp.shape == (s.my1, nx) and np.array_equal(s.stoch_amp, ref)
    assert np.array_equal(s.shell_mode_counts(), ST.mode_counts(nx, ny, Lx, Ly))
    inj = s.stochastic_injection()
    ring = (k >= k_lo) & (k <= k_hi)
    print('%dx%d: %d shells, %d in the ring, %d stored modes forced; sum of the injection / rate - 1 = %.2e'
          % (nx, ny, len(k), ring.sum(), np.count_nonzero(ref), inj.sum() / rate - 1))
    assert inj.dtype == np.float64 and inj.shape == k.shape
    assert abs(inj.sum() - rate) <= 1e-6 * rate                             # the float32 rounding of the table: 6e-8 per entry
    assert not inj[~ring].any() and np.all(inj[ring & (s.shell_mode_counts() > 0)] > 0)
    assert np.allclose(inj, ST.injection(nx, ny, Lx, Ly, ref), rtol=1e-14, atol=0)
    # equal energy per mode: every forced full-spectrum mode gets rate / N
    k2, kept, wt, shell = ST.stored_grid(nx, ny, Lx, Ly)
    e = 0.5 * ref.astype(np.float64) ** 2 / (np.where(kept, k2, 1.0) * float(nx * ny) ** 2)
    N = s.shell_mode_counts()[ring].sum()
    assert np.allclose(e[ref != 0], rate / N, rtol=2e-7, atol=0)
    # per-shell rates, and removal
    by_shell = np.zeros(len(k))
    by_shell[[5, 9]] = 0.25, 0.5
    s.set_stochastic_forcing(by_shell, seed=1)
    assert np.allclose(s.stochastic_injection(), by_shell, rtol=1e-6, atol=0)
    assert s.set_stochastic_forcing(None) is s and s.stoch_amp is None and not s.stochastic_injection().any()


def test_host_refusals():
    from nns.periodic import PeriodicSolver
    s = PeriodicSolver(64, 64, 0.01, 1.0, 0.0)
    S = len(s.shells()[0])
    ok = np.zeros(S)
    ok[4] = 1.0
    for bad in (np.zeros(S - 1), np.zeros((S, 1)), 1.0):
        with pytest.raises(ValueError, match='one entry per shell'):
            s.set_stochastic_forcing(bad)
    for bad in (-ok, np.where(ok > 0, np.nan, 0.0), np.where(ok > 0, np.inf, 0.0)):
        with pytest.raises(ValueError, match='finite and >= 0'):
            s.set_stochastic_forcing(bad)
    with pytest.raises(TypeError, match='rate_by_shell'):
        s.set_stochastic_forcing(['a'] * S)
    empty = np.zeros(S)
    empty[0] = 1.0                                                          # shell 0 holds the (0, 0) mode alone
    with pytest.raises(ValueError, match='no kept mode'):
        s.set_stochastic_forcing(empty)
    for bad in (1.5, '1', True, None):
        with pytest.raises(TypeError, match='seed'):
            s.set_stochastic_forcing(ok, seed=bad)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError, match='seed'):
            s.set_stochastic_forcing(ok, seed=bad)
    assert s.stoch_amp is None                                              # a refused call leaves the solver as it was
    with pytest.raises(ValueError, match='rate'):
        s.ring_forcing(0.0, 4, 6)
    with pytest.raises(TypeError, match='k_lo'):
        s.ring_forcing(1.0, '4', 6)
    with pytest.raises(ValueError, match='no kept mode'):
        s.ring_forcing(1.0, 4.2, 4.8)
    with pytest.raises(ValueError, match='no kept mode'):
        s.ring_forcing(1.0, 100, 200)
    s.set_stochastic_forcing(ok, seed=2 ** 64 - 1)
    assert s.stoch_seed == 2 ** 64 - 1


# ---------------------------------------------------------------------------------------------------- 4. energy from rest
def test_energy_from_rest_grows_at_the_injection_rate():
    # nu = 0, no drag, 64 x 64, ring shells 4..6, B = 16, 50 steps: the truncated nonlinear term conserves energy, the kicks of different steps
    # are independent and E |xi|^2 = 1, so the mean energy is eps t exactly; a grid's energy is a sum over the forced modes of exponential
    # variables of equal mean, so the batch mean has the relative standard deviation 1 / sqrt(N_stored B)
    nx, ny, Lx, Ly = XC.REST
    B, nsteps = 16, 50
    S, amp = XC.rest_scheme(), XC.rest_table()
    eps = ST.injection(nx, ny, Lx, Ly, amp).sum()
    assert abs(eps - XC.REST_RATE) <= 1e-6 * XC.REST_RATE
    X = ST.Stochastic(S, amp, XC.SEED)
    w = X.step(np.zeros((B, nx, ny // 2 + 1), dtype=np.complex128), np.zeros((B, 2)), nsteps)
    E = S.diag(w)[0]
    t = nsteps * XC.REST_DT
    sd = 1.0 / np.sqrt(XC.stored_count(amp) * B)
    print('energy from rest: batch mean %.5f, eps t = %.5f, off by %.2f standard deviations (%.2e relative each)' % (E.mean(), eps * t, (E.mean() / (eps * t) - 1) / sd, sd))
    assert XC.stored_count(amp) == 53
    assert abs(E.mean() / (eps * t) - 1) <= 5 * sd                           # measured: 0.79 standard deviations below


# ---------------------------------------------------------------------------------------------------- 5. mutations
def kick_miss(case, mutate):
    """The worst error of a mutated kick on the forced modes of a kick case, in units of the GPU test's tolerance."""
    nx, ny, B, Lx, Ly = case
    amp = XC.kick_table(case)
    ids = np.arange(min(B, 3))
    ref = ST.kick_stored(nx, ny, XC.KICK_DT, amp, XC.SEED, 0, ids)
    bad = ST.kick_stored(nx, ny, XC.KICK_DT, amp, XC.SEED, 0, ids, mutate)
    xi = ST.xi_stored(nx, ny, XC.SEED, 0, ids, where=amp != 0)
    tol = XC.KICK_TOL * amp.astype(np.float64)[None] * np.sqrt(XC.KICK_DT) * np.maximum(1.0, np.abs(xi))
    m = amp != 0
    return float((np.abs(bad - ref)[:, m] / tol[:, m]).max())


@pytest.mark.parametrize('mutate', ['nosqrtdt', 'var1', 'noconj'])
def test_kick_bound_catches_the_mutations(mutate):
    miss = [kick_miss(c, mutate) for c in XC.KICKS[:2]]
    print('%s: the one-step bound is missed by %s x' % (mutate, ['%.3g' % m for m in miss]))
    assert min(miss) >= 100


def test_moment_bound_catches_variance_one_per_component():
    for case in XC.KICKS:
        m2, m1, bound = XC.moments(XC.kick_samples(case, 'var1')[1])
        assert m2 > 6 * bound, (case, m2, bound)                             # mean |xi|^2 = 2


def test_trajectory_bound_catches_a_kick_before_the_step_and_the_others():
    case = XC.TRAJ[0]
    S, X, (u0, v0), w, _, mean, rate, ratio = XC.reference('flow', case)
    w0 = S.init(u0, v0)[0]
    miss = {}
    for mutate in ST.MUTATIONS:
        bad = ST.Stochastic(S, X.amp, XC.SEED, mutate).step(w0, mean, XC.NSTEPS)
        miss[mutate] = rel_l2c(S.compact(bad), S.compact(w)) / C.BOUND_W
    print('64x64 trajectory, %d steps, injected / initial energy %.2f: BOUND_W is missed by %s' % (XC.NSTEPS, ratio, {k: '%.3g x' % v for k, v in miss.items()}))
    assert min(miss.values()) >= 100
    # without any kick the state is as far away: the noise is comparable to the state, not a perturbation
    plain = S.step(w0, mean, XC.NSTEPS)
    assert rel_l2c(S.compact(plain), S.compact(w)) >= 0.1
    assert 0.99 <= ratio <= 1.01
