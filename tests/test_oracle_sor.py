"""The case table of the lexicographic SOR solve (tests/sor_cases.py) checked without a GPU: the reference arithmetic it leans on, the error
histories that let a tolerance pick its stop sweep, the pipeline every shape is said to take and the batch plan every case is said to run."""
import numpy as np
import pytest

import sor_cases as K
from oracle import chorin_fd as OC

KEYS = sorted(K.NEEDS)
KEY_IDS = [K.shape_id(*k[:3]) + ('' if k[4] == 1 else '-quarter') for k in KEYS]
SMALL = [(3, 3), (3, 7), (7, 3), (4, 5), (6, 11), (12, 5)]


def test_squared_spacings_are_products():
    """make_sor_k multiplies (dx * dx), the oracle writes dx**2: the same double for every spacing the cases use."""
    shapes = {(nx, ny) for nx, ny, *_ in K.SHAPES} | {(nx, ny) for nx, ny, *_ in K.FUSED} | set(SMALL)
    for nx, ny in shapes:
        dx, dy = 2 / (nx - 1), 2 / (ny - 1)
        assert dx ** 2 == dx * dx and dy ** 2 == dy * dy, (nx, ny)
        for dt in (np.float32, np.float64):      # the constants as make_sor_k builds them and as NumPy rounds the oracle's Python floats
            assert dt(2 * (dx * dx) + 2 * (dy * dy)) == dt(2 * dx ** 2 + 2 * dy ** 2) and dt(1 - K.BETA) == dt(-0.25)


@pytest.mark.parametrize('dtype', [K.F64, K.F32])
def test_wavefront_sweep_is_the_lexicographic_sweep_bitwise(dtype):
    """The anti-diagonal order the kernels and the oracle use against the reference's literal double loop, non-square grids, in the type under
    test (a float32 grid stays float32: the Python-float spacings round to the array's type)."""
    for nx, ny in SMALL:
        p0, C, dx, dy = K.problem(nx, ny, dtype, seed=nx * 31 + ny)
        a, b = p0.copy(), p0.copy()
        for _ in range(3):
            OC.sor_sweep_wavefront(a, C, dx, dy, K.BETA)
            OC.sor_sweep_lexicographic(b, C, dx, dy, K.BETA)
            assert a.dtype == b.dtype == np.dtype(dtype)
            assert K.bits(a).tobytes() == K.bits(b).tobytes(), (nx, ny)
        assert np.abs(a - p0).max() > 0


@pytest.mark.parametrize('key', KEYS, ids=KEY_IDS)
def test_error_history_decreases_strictly(key):
    """tol = e_s stops at sweep s only if no earlier error is <= e_s; tol = 0 is never met only while the errors stay positive."""
    errs, snaps = K.history(*key)
    e = np.array(errs, dtype=np.float64)
    assert len(e) == max(K.NEEDS[key]) and np.all(e > 0) and np.all(np.diff(e) < 0), key
    assert set(snaps) == K.NEEDS[key]


def test_history_shortcut_is_the_literal_loop():
    """expected() reads a case's result off its history; the reference's loop itself, run under the case's tol and cap, gives the same."""
    seen = set()
    for c in K.CASES:
        if c.nx * c.ny > 2700 or (c.stop or c.max_sweeps) > 40:
            continue
        p0, C, dx, dy = K.problem(c.nx, c.ny, c.dtype, c.seed, c.scale)
        p, sweeps, err = K.oracle_solve(p0, C, dx, dy, K.BETA, K.tolerance(c), c.max_sweeps)
        n, e, pe = K.expected(c)
        assert sweeps == n and K.bits(err) == K.bits(e) and K.bits(p).tobytes() == K.bits(pe).tobytes(), c
        seen.add(c.kind)
    assert seen == {'stop', 'cap', 'hint'}


def test_one_interior_point_reaches_zero_error():
    """The 3 x 3 grid under tol = 0: the oracle itself says where the loop stops (the error is exactly 0 from some sweep on)."""
    for dtype, sweeps in ((K.F64, 29), (K.F32, 15)):
        p0, C, dx, dy = K.problem(3, 3, dtype)
        p, n, err = K.oracle_solve(p0, C, dx, dy, K.BETA, 0.0, K.MANY)
        assert n == sweeps and err == 0


def test_stated_pipelines_follow_from_the_constants():
    assert K.LDS_HEADER == K.ROWS_BATCH * 8 + 128 and K.LDS_MAX == 153600
    for n, dt, fits in ((9528, K.F64, True), (9529, K.F64, False), (19056, K.F32, True), (19057, K.F32, False)):
        assert K.fits_lds(1, n, dt) == fits
    for nx, ny, dts, pipe, over, stops, _ in K.SHAPES:
        for dt in dts:
            assert K.pipeline(nx, ny, dt) == pipe, (nx, ny, dt)
    assert K.pipeline(8, 1191, K.F64) == 'rows' and K.pipeline(8, 1192, K.F64) == 'global' and 8 * 1191 == 9528
    assert K.pipeline(66, 20, K.F64) == 'rows' and K.pipeline(67, 20, K.F64) == 'lds-fronts'
    for c in K.CASES:
        assert K.pipeline(c.nx, c.ny, c.dtype) == c.pipeline, c
    for nx, ny, dt, _, _ in K.FUSED:
        assert K.fits_lds(nx, ny, dt)
    assert K.uv_fit_lds(70, 68, K.F64) and not K.uv_fit_lds(70, 69, K.F64)
    assert {K.pipeline(nx, ny, dt) for nx, ny, dt, _, _ in K.FUSED} == {'rows', 'lds-fronts'}


def test_stated_batch_plans_are_the_schedule():
    """Every stated plan is what the restated schedule of sor_solve gives for the case's stop, cap and hint."""
    for c in K.CASES:
        assert c.plan == K.plan(c.pipeline, K.first_stop(c), c.max_sweeps, c.hint), c
        if c.plan.stop is not None:
            b, i = c.plan.stop
            assert sum(c.plan.batches[:b]) + i + 1 == c.stop and b == len(c.plan.batches) - 1
            assert c.plan.replay == (i < c.plan.batches[b] - 1)
        assert sum(c.plan.batches) <= c.max_sweeps
    assert K.plan('rows', 0, 40) == K.plan('global', 0, 40) == K.Plan((), None, False, False)        # tol >= the initial err = 1: no batch


def test_the_cases_cover_every_stop_and_every_kind_of_batch():
    for pipe, stops in (('rows', K.ROWS_STOPS), ('lds-fronts', K.FRONT_STOPS), ('global', K.FRONT_STOPS)):
        for dt in (K.F64, K.F32):
            mine = [c for c in K.CASES if c.pipeline == pipe and c.dtype == dt]
            assert {c.stop for c in mine if c.kind == 'stop' and c.plan.stop is not None} >= set(stops), (pipe, dt)
            assert {c.max_sweeps for c in mine if c.kind == 'cap' and c.stop is None} == set(K.CAPS), (pipe, dt)
            assert any(c.stop == c.max_sweeps for c in mine) and any(c.stop is not None and c.stop + 1 == c.max_sweeps for c in mine)
            plans = [c.plan for c in mine]
            stopped = [pl for pl in plans if pl.stop is not None]
            assert any(pl.stop[1] == 0 for pl in stopped), 'a stop at index 0 of a batch'
            assert any(pl.stop[1] == pl.batches[-1] - 1 and not pl.replay for pl in stopped), 'a stop on the last sweep of a batch'
            assert any(0 < pl.stop[1] < pl.batches[-1] - 1 and pl.replay for pl in stopped), 'a stop inside a batch'
            assert any(pl.cut for pl in plans), 'a batch cut short by the cap'
            if pipe == 'rows':
                big = [pl for pl in stopped if pl.batches[pl.stop[0]] == K.ROWS_BATCH and pl.stop[0] >= 2]
                assert {0, K.ROWS_BATCH - 1} <= {pl.stop[1] for pl in big} and any(0 < pl.stop[1] < K.ROWS_BATCH - 1 for pl in big)
                assert any(pl.cut and len(pl.batches) >= 3 for pl in plans), 'a 128-sweep batch cut short by the cap'
    for nx, ny in K.EDGE_SHAPES:
        got = {c.stop for c in K.STOP_CASES if (c.nx, c.ny) == (nx, ny) and c.plan.stop is not None}
        assert got >= set(K.EDGE_STOPS), (nx, ny)
    hints = {(c.stop, c.hint) for c in K.HINT_CASES}
    for s in (9, 40):
        assert {h for st, h in hints if st == s} == {s, s - 1, s + 1, 128, 129, 1000}
    assert all(c.pipeline == 'rows' for c in K.HINT_CASES)


@pytest.mark.parametrize('shape', K.BATCH_SHAPES, ids=[K.shape_id(*s) for s in K.BATCH_SHAPES])
def test_batch_grids_stop_at_different_sweeps(shape):
    nx, ny, dt = shape
    p0, C, dx, dy = K.problem(nx, ny, dt)
    tol = float(K.history(nx, ny, dt)[0][K.BATCH_STOP - 1])
    T = np.dtype(dt).type
    sweeps = [K.oracle_solve(p0 * T(s), C, dx, dy, K.BETA, tol, K.BATCH_CAP)[1] for s in K.BATCH_SCALES]
    assert sweeps[0] == K.BATCH_STOP and sweeps[2] == K.BATCH_CAP and abs(sweeps[1] - K.BATCH_STOP) <= 2, sweeps
