"""The float64 restatement of the reverse mode of particle sampling (tests/pspec_particles_adjoint_oracle.py) checked on the CPU: (i) its
spread and its coefficient transpose are the transposes of the gather and the coefficient build to round-off; (ii) every gradient of
``observe`` equals central differences of the restated forward, also at points on a node and astride a cell boundary; (iii) on the GPU
test's own cases every deliberately wrong variant lies at least 10x the GPU bound of its quantity away from the right one."""
import numpy as np
import pytest

import pspec_particles_adjoint_cases as AC
import pspec_particles_adjoint_oracle as AO
import pspec_particles_oracle as PO


def dot(a, b):
    return float(np.sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)))


# ---------------------------------------------------------------------------------------------------- (i) transposes
@pytest.mark.parametrize('order', AC.ORDERS)
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_spread_is_the_transpose_of_the_gather(shape, order):
    nx, ny, Lx, Ly = shape
    rng = np.random.default_rng(11)
    for name in ('mixed', 'cluster'):
        pos = AC.positions(shape, 3, name)
        x, y = pos[..., 0], pos[..., 1]
        c, r = rng.standard_normal((3, nx, ny)), rng.standard_normal(x.shape)
        lhs, rhs = dot(PO.evaluate(c, x, y, Lx, Ly, order), r), dot(c, AO.spread(r, x, y, nx, ny, Lx, Ly, order))
        size = np.linalg.norm(PO.evaluate(c, x, y, Lx, Ly, order)) * np.linalg.norm(r)
        assert abs(lhs - rhs) <= 1e-12 * size, (name, lhs, rhs)


@pytest.mark.parametrize('order', AC.ORDERS)
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_the_coefficient_transpose_is_the_transpose_of_the_build(shape, order):
    nx, ny, Lx, Ly = shape
    rng = np.random.default_rng(12)
    w, th = rng.standard_normal((2, nx, ny)), rng.standard_normal((2, nx, ny))          # white: every mode of the band and beyond it
    r = {f: rng.standard_normal((2, nx, ny)) for f in AC.ALL}
    coef = AO.build(w, th, None, Lx, Ly, order)
    wbar, thbar = AO.build_adjoint(r, Lx, Ly, order)
    lhs, rhs = sum(dot(coef[f], r[f]) for f in AC.ALL), dot(w, wbar) + dot(th, thbar)
    size = np.sqrt(sum(np.linalg.norm(coef[f]) ** 2 for f in AC.ALL)) * np.sqrt(sum(np.linalg.norm(r[f]) ** 2 for f in AC.ALL))
    assert abs(lhs - rhs) <= 1e-12 * size, (lhs, rhs)
    # a subset of the fields, each alone
    for f in AC.ALL:
        wb, tb = AO.build_adjoint({f: r[f]}, Lx, Ly, order)
        rhs = dot(th, tb) if f == 'theta' else dot(w, wb)
        assert abs(dot(coef[f], r[f]) - rhs) <= 1e-12 * np.linalg.norm(coef[f]) * np.linalg.norm(r[f]), f
        assert (wb is None) == (f == 'theta') and (tb is None) == (f != 'theta')


def test_the_restated_build_is_the_tracers_restatement():
    """``build`` from fields agrees with pspec_particles_oracle.Tracers.coefficients from the flow restatement's spectra."""
    import pspec_particles_cases as PC
    shape = PC.OBLONG
    nx, ny, Lx, Ly = shape
    S, w, mean, t = PC.start('buoyant', shape)
    for order in AC.ORDERS:
        ref = PO.Tracers(S, order).coefficients(w, mean, t, AC.ALL)
        got = AO.build(np.fft.irfft2(w, s=(nx, ny)), np.fft.irfft2(t, s=(nx, ny)), mean, Lx, Ly, order)
        for k, f in enumerate(AC.ALL):
            assert np.abs(got[f] - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), (order, f)


def test_the_derivative_weights_are_the_weights_derivatives():
    t = np.linspace(0.0, 1.0, 41)[1:-1]
    for order in AC.ORDERS:
        fd = (PO.weights(t + 1e-5, order) - PO.weights(t - 1e-5, order)) / 2e-5          # truncation ~ 2e-10, round-off about the same
        assert np.abs(AO.dweights(t, order) - fd).max() <= 1e-9
        # the weights sum to one; the middle piece's terms reach 450 x^2 / 120 ~ 15 at x = 2: a dozen roundings of that size
        assert np.abs(AO.dweights(t, order).sum(axis=0)).max() <= 1e-13
        # continuous across a cell boundary: node a at t = 1 is node a - 1 of the next cell at t = 0, and the node that leaves has weight 0
        assert np.abs(AO.dweights(1.0, order)[1:] - AO.dweights(0.0, order)[:-1]).max() <= 1e-15
        assert AO.dweights(1.0, order)[0] == 0.0 and AO.dweights(0.0, order)[-1] == 0.0


# ---------------------------------------------------------------------------------------------------- (ii) gradients against differences
def _special_points(shape):
    """[2, P, 2]: on a node (t = 0), pairs astride a cell boundary, the first and last cells, generic points."""
    nx, ny, Lx, Ly = shape
    hx, hy = Lx / nx, Ly / ny
    one = [(5 * hx, 7 * hy), (0.0, 0.0), (9 * hx - 1e-7, 3 * hy + 1e-7), (9 * hx + 1e-7, 3 * hy - 1e-7), (0.4 * hx, (ny - 0.3) * hy),
           ((nx - 0.2) * hx, 0.6 * hy), (-2.3 * hx, Ly + 1.7 * hy), (20.37 * hx, 31.61 * hy)]
    return np.array([one, [(x + 0.13, y - 0.29) for x, y in one]])


@pytest.mark.parametrize('order', AC.ORDERS)
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_the_gradients_of_observe_match_central_differences(shape, order):
    nx, ny, Lx, Ly = shape
    w, th = (a[:2].astype(np.float64) for a in AC.fields(shape, 3))
    mean = AC.MEANS[:2]
    pos = _special_points(shape)
    x, y = pos[..., 0], pos[..., 1]
    rng = np.random.default_rng(13)
    r = rng.standard_normal(x.shape + (4,))
    loss = lambda w_, th_: dot(AO.observe(w_, th_, mean, x, y, AC.ALL, Lx, Ly, order), r)
    wbar, thbar, xbar, ybar = AO.observe_gradients(w, th, mean, x, y, AC.ALL, r, Lx, Ly, order)
    # w and theta: the loss is linear in them, so a difference along a direction is exact to round-off
    d = rng.standard_normal(w.shape)
    for name, bar, fd in (('w', wbar, (loss(w + d, th) - loss(w - d, th)) / 2.0), ('theta', thbar, (loss(w, th + d) - loss(w, th - d)) / 2.0)):
        assert abs(fd - dot(bar, d)) <= 1e-8 * np.linalg.norm(bar) * np.linalg.norm(d), (name, fd, dot(bar, d))
    # x and y: each point alone, central differences with a step well inside a cell.  The splines are C^2 (C^4): the one-sided third
    # derivative jumps at a boundary, so astride one the difference is good to O(step^2 jump / 6), inside the bound
    # (a point's values depend on its own position alone, so all points move at once and every point's own sum is differenced)
    step = 1e-5 * min(Lx / nx, Ly / ny)
    coef = AO.build(w, th, mean, Lx, Ly, order)
    own = lambda x_, y_: sum(r[..., k] * PO.evaluate(coef[f], x_, y_, Lx, Ly, order) for k, f in enumerate(AC.ALL))
    for name, bar, e in (('x', xbar, (step, 0.0)), ('y', ybar, (0.0, step))):
        fd = (own(x + e[0], y + e[1]) - own(x - e[0], y - e[1])) / (2 * step)
        assert np.abs(fd - bar).max() <= 1e-8 * np.abs(bar).max(), (name, np.abs(fd - bar).max(), np.abs(bar).max())
    # shared points: the gradient is the sum over the grids
    sb = AO.observe_gradients(w, th, mean, x[0], y[0], AC.ALL, r, Lx, Ly, order)
    each = AO.observe_gradients(w, th, mean, np.stack([x[0], x[0]]), np.stack([y[0], y[0]]), AC.ALL, r, Lx, Ly, order)
    assert np.allclose(sb[2], each[2].sum(axis=0), rtol=0, atol=1e-13 * np.abs(each[2]).max())
    assert np.allclose(sb[3], each[3].sum(axis=0), rtol=0, atol=1e-13 * np.abs(each[3]).max())


# ---------------------------------------------------------------------------------------------------- (iii) the wrong variants
@pytest.mark.parametrize('wrong', AO.WRONG)
def test_every_wrong_variant_is_told_apart_on_the_gpu_cases(wrong):
    for shape in AC.SHAPES:
        for order in AC.ORDERS:
            right, bad = AC.reference(shape, 3, 'mixed', order), AC.reference(shape, 3, 'mixed', order, wrong)
            for q in AC.SHOWS[wrong]:
                e = AC.rel_l2(bad[q], right[q])
                assert e >= 10 * AC.BOUND[q], (wrong, AC.shape_id(shape), order, q, e)


def test_the_bounds_respect_their_caps_and_their_measurements():
    assert AC.CAP == 1e-5 and set(AC.BOUND) == set(AC.MEASURED)
    for q, b in AC.BOUND.items():
        assert b <= (1e-6 if q in ('identity', 'chain') else AC.CAP), q
        if q in AC.AT_THE_CAP:                            # 4x would pass the cap: the bound is the cap, never more, and the figure lies below it
            assert b == AC.CAP and AC.MEASURED[q] < AC.CAP < 4 * AC.MEASURED[q], q
        else:
            assert 3.9 * AC.MEASURED[q] <= b <= 4.1 * AC.MEASURED[q], q


def test_the_cell_keys_name_the_cell_of_the_gather():
    nx, ny, Lx, Ly = shape = AC.OBLONG
    pos = AC.positions(shape, 3, 'mixed')
    key = AO.cell_keys(pos[..., 0], pos[..., 1], nx, ny, Lx, Ly)
    assert key.min() >= 0 and np.all(key // (nx * ny) == np.arange(3)[:, None])
    i0 = AO.locate(pos[..., 0], Lx / nx, nx, 6)[0]
    assert np.all((key // ny) % nx == (i0 + 2) % nx)
    cl = AC.positions(shape, 3, 'cluster')
    assert len(np.unique(AO.cell_keys(cl[..., 0], cl[..., 1], nx, ny, Lx, Ly) % (nx * ny))) == 1
