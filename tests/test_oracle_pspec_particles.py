"""The float64 restatement of the Lagrangian tracers (tests/pspec_particles_oracle.py) on the CPU: the splines against the exact Fourier sum,
the order of the two time schemes, and the reach of the GPU bounds (tests/pspec_particles_cases.py) -- every deliberately wrong variant lies
>= 10x the bound it is held to away from the right one, on the GPU test's own inputs."""
import numpy as np
import pytest

import pspec_oracle as O
import pspec_particles_cases as PC
import pspec_particles_oracle as PO


def random_spectrum(nx, ny, seed, mmax=8):
    """The rfft2 spectrum of a random real field with |m_x|, |m_y| <= mmax and a mean."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((nx, ny))
    fh = np.fft.rfft2(f)
    mx = np.abs(np.fft.fftfreq(nx) * nx)
    fh *= (mx[:, None] <= mmax) & (np.arange(ny // 2 + 1)[None, :] <= mmax)
    return fh


def spline_error(n, order, seed=11):
    """max |spline - exact| / max |f| at 400 unwrapped points in +-3 boxes.  The field is the same at every n: its modes are drawn at 64^2."""
    L = 2 * np.pi
    f64 = random_spectrum(64, 64, seed)
    fh = np.zeros((n, n // 2 + 1), dtype=complex)
    for i in range(64):
        m = i if i < 32 else i - 64
        if abs(m) <= 8:
            fh[m % n, :9] = f64[i, :9] * (n / 64.0) ** 2
    rng = np.random.default_rng(seed + 1)
    x, y = rng.uniform(-3 * L, 3 * L, 400), rng.uniform(-3 * L, 3 * L, 400)
    ref = PO.exact(fh, x, y, n, n, L, L)
    got = PO.evaluate(PO.coefficients(fh, n, n, order), x, y, L, L, order)
    return np.abs(got - ref).max() / np.abs(np.fft.irfft2(fh, s=(n, n))).max()


def test_weights_are_a_partition_of_unity():
    t = np.linspace(0.0, 1.0, 1001)
    for order in PC.ORDERS:
        w = PO.weights(t, order)
        assert w.shape == (order, 1001) and np.abs(w.sum(axis=0) - 1.0).max() < 4e-15
        assert w.min() >= 0.0
        # the symbol is the weights' transform at the nodes: beta(theta) = sum_j B(j) cos(j theta)
        th = np.linspace(0, np.pi, 9)
        nodes = PO.weights(0.0, order)
        first = order // 2 - 1
        sym = sum(nodes[a] * np.cos((a - first) * th) for a in range(order))
        assert np.abs(sym - PO.beta(th, order)).max() < 1e-15


def test_exact_sum_is_the_inverse_transform_at_the_nodes():
    nx, ny, Lx, Ly = 64, 128, 2 * np.pi, 5.0
    fh = random_spectrum(nx, ny, 5)
    f = np.fft.irfft2(fh, s=(nx, ny))
    i, j = np.array([0, 3, 63, 17]), np.array([0, 127, 64, 5])
    assert np.abs(PO.exact(fh, i * Lx / nx - 2 * Lx, j * Ly / ny + 3 * Ly, nx, ny, Lx, Ly) - f[i, j]).max() < 1e-13 * np.abs(f).max()
    for order in PC.ORDERS:                                               # and the spline interpolates: it returns the samples at the nodes
        got = PO.evaluate(PO.coefficients(fh, nx, ny, order), i * Lx / nx, j * Ly / ny, Lx, Ly, order)
        assert np.abs(got - f[i, j]).max() < 1e-13 * np.abs(f).max()


def test_spline_against_exact_sum():
    e4, e6 = [spline_error(n, 4) for n in (64, 128)], [spline_error(n, 6) for n in (64, 128)]
    print('order 4: %.2e %.2e   order 6: %.2e %.2e' % (e4[0], e4[1], e6[0], e6[1]))
    assert e4[0] <= 1e-3 and e6[0] <= 3e-5
    assert e4[0] / e4[1] >= 12 and e6[0] / e6[1] >= 48


def steady_flow(kind, dt):
    """(scheme, w, mean) of a steady inviscid flow at 64^2: a single-mode shear with a mean flow along it, or the Taylor-Green cell."""
    n = 64
    S = O.Scheme(n, n, dt, 1.0, 0.0)
    X, Y = np.meshgrid(2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(n) / n, indexing='ij')
    if kind == 'shear':
        return (S,) + S.init(0.4 + 0.8 * np.sin(2 * Y), np.zeros_like(X))
    u, v, _ = O.taylor_green(n, n, 0.0, 0.0)
    return (S,) + S.init(u, v)


def start_points():
    rng = np.random.default_rng(3)
    return rng.uniform(-2 * np.pi, 4 * np.pi, (40, 2))


def test_a_steady_shear_carries_particles_along_straight_lines():
    """u = U0 + A sin(k y), v = 0: the velocity is constant along a trajectory, which both schemes then integrate exactly at any dt, so there
    is no error whose fall could be measured; the positions are the analytic ones to rounding."""
    pos0 = start_points()
    for scheme, nsteps in (('rk4', 8), ('heun', 7)):
        for dt in (0.1, 0.05):
            S, w, mean = steady_flow('shear', dt)
            pos = PO.Tracers(S, sampler='exact').advect(w, mean, pos0, nsteps, scheme)[2]
            ref = pos0 + nsteps * dt * np.stack([0.4 + 0.8 * np.sin(2 * pos0[:, 1]), np.zeros(len(pos0))], axis=-1)
            assert np.abs(pos - ref).max() < 1e-12


def trajectory_errors(scheme, dts, T=0.8):
    pos0 = start_points()
    end = {}
    for dt in dts + (dts[-1] / 4,):
        S, w, mean = steady_flow('tg', dt)
        end[dt] = PO.Tracers(S, sampler='exact').advect(w, mean, pos0, int(round(T / dt)), scheme)[2]
    ref = end[dts[-1] / 4]
    return [np.abs(end[dt] - ref).max() for dt in dts]


def test_rk4_is_fourth_order_on_the_taylor_green_cell():
    e = trajectory_errors('rk4', (0.1, 0.05, 0.025))                     # particle steps H = 2 dt
    print('rk4 errors', e)
    assert e[0] / e[1] >= 14 and e[1] / e[2] >= 14


def test_heun_is_second_order_on_the_taylor_green_cell():
    e = trajectory_errors('heun', (0.1, 0.05, 0.025))
    print('heun errors', e)
    assert e[0] / e[1] >= 3.5 and e[1] / e[2] >= 3.5


# ---------------------------------------------------------------------------------------------------- the reach of the GPU bounds
@pytest.mark.parametrize('order', PC.ORDERS)
@pytest.mark.parametrize('wrong', PO.SAMPLING)
def test_the_sample_bound_tells_every_wrong_read_apart(wrong, order):
    right, bad = PC.oracle_read(PC.SQUARE, order)[1], PC.oracle_read(PC.SQUARE, order, wrong)[1]
    fields = ('u', 'v') if wrong == 'no_mean' else ('u', 'v', 'w')
    far = min(PC.rel_max(bad[f], right[f]) for f in fields)
    print(wrong, order, far)
    assert far >= 10 * PC.SAMPLE_BOUND


@pytest.mark.parametrize('wrong', ('unfiltered',))
@pytest.mark.parametrize('order', PC.ORDERS)
def test_the_coefficient_bound_tells_a_missing_prefilter_apart(wrong, order):
    right, bad = PC.oracle_read(PC.SQUARE, order)[0], PC.oracle_read(PC.SQUARE, order, wrong)[0]
    assert min(PC.rel_max(bad[f], right[f]) for f in ('u', 'v', 'w', 'theta')) >= 10 * PC.COEF_BOUND


@pytest.mark.parametrize('scheme,nsteps', PC.SCHEMES)
@pytest.mark.parametrize('wrong', PO.WRONG)
def test_the_advect_bound_tells_every_wrong_variant_apart(wrong, scheme, nsteps):
    pos0 = PC.positions(PC.SQUARE)
    right = PC.oracle_advect('plain', PC.SQUARE, scheme, nsteps, 4)
    bad = PC.oracle_advect('plain', PC.SQUARE, scheme, nsteps, 4, wrong)
    far = PC.displacement_error(bad, right, pos0)
    print(wrong, scheme, far)
    assert far >= 10 * PC.ADVECT_BOUND


def test_the_cases_name_the_fields_in_the_order_of_the_mask():
    """Bit k of the C entries' field mask is field k of the cases, and the solver has the calls the GPU test makes (no GPU used)."""
    from nns import ops
    from nns.periodic import PeriodicParticles, PeriodicSolver
    assert tuple(ops.PARTICLE_FIELDS) == PC.FIELDS
    for name in ('init_particles', 'particle_coefficients', 'sample', 'advect'):
        assert callable(getattr(PeriodicSolver, name)), name
    assert all(callable(getattr(PeriodicParticles, name)) for name in ('clone', 'wrapped'))
    s = PC.solver('buoyant', PC.SQUARE)
    mask, slots = s._field_mask(('theta', 'u', 'u', 'w'), type('S', (), dict(that=object()))())
    assert mask == 0b1101 and slots == [2, 0, 0, 1]
    with pytest.raises(ValueError, match='theta'):
        s._field_mask(('theta',), type('S', (), dict(that=None))())


def test_the_bounds_are_those_measured():
    """Each bound is 4x the largest error seen on the MI355X (MEASURED), no more."""
    for name, bound in (('coef', PC.COEF_BOUND), ('sample', PC.SAMPLE_BOUND), ('advect', PC.ADVECT_BOUND)):
        assert PC.MEASURED[name] is not None and bound <= 4.0 * PC.MEASURED[name] * 1.0001, name
