"""Cases of the lexicographic SOR solve (nns_fd_sor_*, csrc/sor_device.h: sor_solve) for tests/test_gpu_sor.py (on the GPU, bitwise against
oracle/chorin_fd.py) and tests/test_oracle_sor.py (on the CPU: the table is what it says it is).

One function, sor_solve, picks one of three pipelines, restated here from csrc/sor_device.h:
  'rows'        p and C fit one workgroup's LDS and nx - 2 <= 64: one lane per row (sor_batch_rows)
  'lds-fronts'  they fit and nx - 2 > 64: anti-diagonal fronts, 16 sweeps in flight (sor_batch on LDS)
  'global'      they do not fit: sor_batch on the grid in global memory
and runs the sweeps in speculative batches: batch 0 has `hint` sweeps (16 without a hint), batch 1 has 16, later ones 128 on the rows
pipeline and always 16 on the other two; every batch is cut to the sweeps the cap leaves.  A sweep inside a batch that meets the tolerance
costs a restore and a replay of the sweeps up to it; a stop on the last sweep of a batch does not.  No batch runs when the tolerance is at
or above the initial err = 1.

Every problem is  rng = default_rng(seed); dx, dy = 2 / (nx - 1), 2 / (ny - 1); p0 = 0.5 N(0, 1); C = N(0, 1) dx dy; beta = 1.25.  Its
per-sweep error e_1, e_2, ... decreases strictly as far as the cases look (tests/test_oracle_sor.py asserts it), so tol = float(e_s) stops
the solve at sweep s exactly, on the err == tol edge of the loop's `err > tol` -- unless e_s >= 1: the loop compares the INITIAL err = 1 with
tol first, so such a tolerance means no sweep at all.  On most shapes e_1 (2 .. 3) and e_2 (1.0 .. 1.5) are that large.  Those cases stay
as they are, with the oracle's answer (0 sweeps, p untouched), and each has a twin on the problem scaled by 1/4 (p0 and C; a power of two,
so the history is the same one with every error exactly a quarter: e_1 <= 0.74), which does stop at sweep s.
"""
import collections
import functools

import numpy as np

from oracle import chorin_fd as OC

F64, F32 = 'float64', 'float32'
BETA = 1.25
MANY = 300                                   # the sweep cap of a case that is to stop on its tolerance

# csrc/sor_device.h
WAVE = 64                                    # lanes of a wave: the rows pipeline needs nx - 2 <= WAVE
WAVES = 16                                   # kSorWaves: sweeps of a batch of the front pipelines, and of the second batch everywhere
ROWS_BATCH = 128                             # kSorBatch: the rows pipeline's later batches
LDS_HEADER = 1152                            # kSorHdr = kSorBatch * 8 + 128
LDS_MAX = 150 * 1024                         # kSorLdsMax


def fits_lds(nx, ny, dtype):
    """p and C in one workgroup's LDS: nx ny <= 9528 in float64, <= 19056 in float32."""
    return LDS_HEADER + 2 * nx * ny * np.dtype(dtype).itemsize <= LDS_MAX


def uv_fit_lds(nx, ny, dtype):
    """The fused explicit step keeps the intermediate velocities in LDS as well (UV_LDS, csrc/fd_step_kernels.hip)."""
    return LDS_HEADER + 4 * nx * ny * np.dtype(dtype).itemsize <= LDS_MAX


def pipeline(nx, ny, dtype):
    if not fits_lds(nx, ny, dtype):
        return 'global'
    return 'rows' if nx - 2 <= WAVE else 'lds-fronts'


# batches: the sweeps of every batch run; stop: (batch, index in it) of the sweep that meets the tolerance, None when the cap ends the solve;
# replay: the stop is not the last sweep of its batch; cut: the cap shortened the last batch
Plan = collections.namedtuple('Plan', 'batches stop replay cut')


def plan(pipe, stop_sweep, max_sweeps, hint=0):
    """sor_solve's schedule.  stop_sweep: the first sweep (from 1) whose error is <= tol, 0 when the initial err = 1 already is, None for never."""
    if stop_sweep == 0:
        return Plan((), None, False, False)
    done, batches, cut = 0, [], False
    while done < max_sweeps:
        want = (hint if hint >= 1 else WAVES) if not batches else WAVES if len(batches) == 1 else ROWS_BATCH
        full = min(want, ROWS_BATCH) if pipe == 'rows' else WAVES
        nsw = min(full, max_sweeps - done)
        cut = nsw < full
        batches.append(nsw)
        if stop_sweep is not None and stop_sweep <= done + nsw:
            idx = stop_sweep - done - 1
            return Plan(tuple(batches), (len(batches) - 1, idx), idx < nsw - 1, cut)
        done += nsw
    return Plan(tuple(batches), None, False, cut)


# ---------------------------------------------------------------------------------------------------- stops: tol = e_s, cap MANY
ROWS_STOPS = (1, 2, 16, 17, 31, 32, 33, 100, 160, 161)      # first, middle, last sweep of batches 0, 1, 2 and the first of batch 3
FRONT_STOPS = (1, 15, 16, 17, 32, 33, 40)
EDGE_STOPS = (1, 16, 17, 33)

_R, _F = (WAVES, WAVES, ROWS_BATCH, ROWS_BATCH), (WAVES, WAVES, WAVES)
STOP_PLANS = {
    'rows': {
        1: Plan(_R[:1], (0, 0), True, False), 2: Plan(_R[:1], (0, 1), True, False), 5: Plan(_R[:1], (0, 4), True, False),
        16: Plan(_R[:1], (0, 15), False, False), 17: Plan(_R[:2], (1, 0), True, False), 31: Plan(_R[:2], (1, 14), True, False),
        32: Plan(_R[:2], (1, 15), False, False), 33: Plan(_R[:3], (2, 0), True, False), 100: Plan(_R[:3], (2, 67), True, False),
        160: Plan(_R[:3], (2, 127), False, False), 161: Plan(_R, (3, 0), True, False)},
    'fronts': {
        1: Plan(_F[:1], (0, 0), True, False), 15: Plan(_F[:1], (0, 14), True, False), 16: Plan(_F[:1], (0, 15), False, False),
        17: Plan(_F[:2], (1, 0), True, False), 32: Plan(_F[:2], (1, 15), False, False), 33: Plan(_F, (2, 0), True, False),
        40: Plan(_F, (2, 7), True, False)},
}
STOP_PLANS['lds-fronts'] = STOP_PLANS['global'] = STOP_PLANS['fronts']

# nx, ny, types, pipeline, the number of leading errors e_1, .. that are >= 1 (the initial err), stops, the edge the shape exercises
SHAPES = [
    (3, 3, (F64, F32), 'rows', 0, (1, 2, 5), 'one interior point (its error reaches 0 at sweep 29 / 15: stops at s <= 5 only)'),
    (3, 40, (F64, F32), 'rows', 1, EDGE_STOPS, 'one interior row: lane 0 alone'),
    (40, 3, (F64, F32), 'rows', 0, EDGE_STOPS, 'one interior column: every point is a first and a last column'),
    (4, 5, (F64, F32), 'rows', 1, (1, 2, 5, 16), 'smallest general grid (its float32 error stops decreasing after sweep 17)'),
    (35, 52, (F64, F32), 'rows', 2, ROWS_STOPS, 'general non-square grid'),
    (51, 51, (F64, F32), 'rows', 2, ROWS_STOPS, "the reference's grid"),
    (64, 64, (F64, F32), 'rows', 2, (1, 16, 33, 160), 'BASELINE config 1'),
    (66, 5, (F64, F32), 'rows', 2, EDGE_STOPS + (161,), 'all 64 lanes, fewer columns than the lag between sweeps'),
    (66, 66, (F64, F32), 'rows', 2, ROWS_STOPS, 'all 64 lanes, square'),
    (5, 66, (F64, F32), 'rows', 1, EDGE_STOPS + (160,), 'P = ny - 2 > 48 with three rows'),
    (10, 200, (F64, F32), 'rows', 1, ROWS_STOPS, 'P = ny - 2 > 48 with eight rows'),
    (66, 144, (F64, F32), 'rows', 2, EDGE_STOPS + (100, 161), '9504 points: at the float64 LDS cap with every lane busy'),
    (8, 1191, (F64,), 'rows', 2, EDGE_STOPS, 'exactly 9528 points: the float64 LDS boundary'),
    (66, 288, (F32,), 'rows', 2, EDGE_STOPS + (161,), '19008 points: at the float32 LDS cap'),
    (67, 20, (F64, F32), 'lds-fronts', 2, FRONT_STOPS, '65 interior rows: one past the rows pipeline'),
    (130, 20, (F64, F32), 'lds-fronts', 2, FRONT_STOPS, 'many rows, few columns'),
    (80, 80, (F64, F32), 'lds-fronts', 2, FRONT_STOPS, 'fronts longer than a wave'),
    (67, 142, (F64, F32), 'lds-fronts', 2, EDGE_STOPS + (40,), '9514 points: near the float64 LDS cap'),
    (137, 139, (F32,), 'lds-fronts', 2, FRONT_STOPS, '19043 points: near the float32 LDS cap'),
    (8, 1192, (F64,), 'global', 2, EDGE_STOPS, 'one column past the float64 LDS boundary'),
    (100, 96, (F64,), 'global', 2, FRONT_STOPS, '9600 points: just past the float64 LDS cap'),
    (140, 137, (F32,), 'global', 2, FRONT_STOPS, '19180 points: just past the float32 LDS cap'),
]
EDGE_SHAPES = ((3, 40), (40, 3), (66, 5), (66, 66), (10, 200), (8, 1191), (8, 1192))     # these meet at least EDGE_STOPS

# kind 'stop' / 'cap' / 'hint'; stop: the sweep whose error is the tolerance, None for tol = 0; pipeline and plan: what the case is to run
# scale: of p0 and C (1: the recipe itself)
Case = collections.namedtuple('Case', 'kind nx ny dtype seed stop max_sweeps hint pipeline plan scale', defaults=(1.0,))
NO_SWEEP = Plan((), None, False, False)
QUARTER = 0.25

STOP_CASES = [Case('stop', nx, ny, dt, 0, s, MANY, 0, pipe, NO_SWEEP if s <= over else STOP_PLANS[pipe][s])
              for nx, ny, dts, pipe, over, stops, _ in SHAPES for dt in dts for s in stops]
STOP_CASES += [Case('stop', nx, ny, dt, 0, s, MANY, 0, pipe, STOP_PLANS[pipe][s], QUARTER)
               for nx, ny, dts, pipe, over, stops, _ in SHAPES for dt in dts for s in stops if s <= over]

# ---------------------------------------------------------------------------------------------------- caps
# tol = 0 is never met (the histories stay positive): the cap ends the solve
CAPS = (0, 1, 15, 16, 17, 40, 161)
CAP_PLANS = {
    'rows': {0: Plan((), None, False, False), 1: Plan((1,), None, False, True), 15: Plan((15,), None, False, True),
             16: Plan((16,), None, False, False), 17: Plan((16, 1), None, False, True), 40: Plan((16, 16, 8), None, False, True),
             161: Plan((16, 16, 128, 1), None, False, True)},
    'fronts': {0: Plan((), None, False, False), 1: Plan((1,), None, False, True), 15: Plan((15,), None, False, True),
               16: Plan((16,), None, False, False), 17: Plan((16, 1), None, False, True), 40: Plan((16, 16, 8), None, False, True),
               161: Plan((16,) * 10 + (1,), None, False, True)},
}
CAP_PLANS['lds-fronts'] = CAP_PLANS['global'] = CAP_PLANS['fronts']
# tol = e_s with the cap at s (stop and cap coincide: the stop is the last sweep of a batch the cap cut) and at s + 1
COINCIDE_PLANS = {
    'rows': {(17, 17): Plan((16, 1), (1, 0), False, True), (17, 18): Plan((16, 2), (1, 0), True, True),
             (100, 100): Plan((16, 16, 68), (2, 67), False, True), (100, 101): Plan((16, 16, 69), (2, 67), True, True)},
    'fronts': {(17, 17): Plan((16, 1), (1, 0), False, True), (17, 18): Plan((16, 2), (1, 0), True, True),
               (40, 40): Plan((16, 16, 8), (2, 7), False, True), (40, 41): Plan((16, 16, 9), (2, 7), True, True)},
}
COINCIDE_PLANS['lds-fronts'] = COINCIDE_PLANS['global'] = COINCIDE_PLANS['fronts']
CAP_SHAPES = [(51, 51, F64), (51, 51, F32), (40, 3, F64), (67, 20, F64), (67, 20, F32), (100, 96, F64), (140, 137, F32)]

CAP_CASES = [Case('cap', nx, ny, dt, 0, None, m, 0, pipeline(nx, ny, dt), CAP_PLANS[pipeline(nx, ny, dt)][m])
             for nx, ny, dt in CAP_SHAPES for m in CAPS]
CAP_CASES += [Case('cap', nx, ny, dt, 0, s, m, 0, pipeline(nx, ny, dt), pl)
              for nx, ny, dt in CAP_SHAPES for (s, m), pl in COINCIDE_PLANS[pipeline(nx, ny, dt)].items()]

# ---------------------------------------------------------------------------------------------------- hints (rows pipeline)
# the hint sizes batch 0 (at most 128 sweeps); the result must not depend on it: a stop inside and one beyond the first 16 sweeps
HINT_PLANS = {
    (9, 9): Plan((9,), (0, 8), False, False), (9, 8): Plan((8, 16), (1, 0), True, False), (9, 10): Plan((10,), (0, 8), True, False),
    (9, 128): Plan((128,), (0, 8), True, False), (9, 129): Plan((128,), (0, 8), True, False), (9, 1000): Plan((128,), (0, 8), True, False),
    (40, 40): Plan((40,), (0, 39), False, False), (40, 39): Plan((39, 16), (1, 0), True, False), (40, 41): Plan((41,), (0, 39), True, False),
    (40, 128): Plan((128,), (0, 39), True, False), (40, 129): Plan((128,), (0, 39), True, False),
    (40, 1000): Plan((128,), (0, 39), True, False),
}
HINT_SHAPES = [(51, 51, F64), (51, 51, F32), (5, 66, F64), (66, 5, F32)]
HINT_CASES = [Case('hint', nx, ny, dt, 0, s, MANY, h, 'rows', pl) for nx, ny, dt in HINT_SHAPES for (s, h), pl in HINT_PLANS.items()]

CASES = STOP_CASES + CAP_CASES + HINT_CASES

# ---------------------------------------------------------------------------------------------------- batches and special values
# B = 3 grids in one launch: one C, p0 scaled by 1, 1e-3, 1e3, one tol = e_20 of the unscaled grid, cap 60.  The 1e3 grid runs to the cap; C
# carries as much of the error as p0 does, so the 1e-3 grid stops with the unscaled one or a sweep after it.
BATCH_SCALES = (1.0, 1e-3, 1e3)
BATCH_STOP, BATCH_CAP = 20, 60
BATCH_SHAPES = [(35, 52, F64), (35, 52, F32), (67, 20, F64), (67, 20, F32), (100, 96, F64), (140, 137, F32)]
# tol >= the initial err = 1 (no sweep at all), all zeros, signed zeros, one NaN: once per pipeline and type
SPECIAL_SHAPES = [(35, 52, F64), (66, 5, F32), (67, 20, F64), (80, 80, F32), (100, 96, F64), (140, 137, F32)]

# the fused explicit step (nns_fd_step_explicit_*) on non-square grids: nx, ny, type, corrected advection, the edge
FUSED = [
    (40, 56, F64, False, 'general non-square grid'),
    (66, 20, F64, False, 'non-square grid with all 64 lanes'),
    (20, 66, F64, True, 'its transpose, with the corrected advection'),
    (67, 20, F32, False, 'lds-fronts inside the fused kernel'),
    (70, 68, F64, False, '4760 points: the intermediate velocities still fit LDS'),
    (70, 69, F64, False, '4830 points: they no longer fit'),
]


def shape_id(nx, ny, dtype):
    return '%dx%d-%s' % (nx, ny, 'f64' if dtype == F64 else 'f32')


# ---------------------------------------------------------------------------------------------------- problems and the reference
def problem(nx, ny, dtype, seed=0, scale=1.0):
    """p0, C (in dtype), dx, dy (Python floats) of a case."""
    rng = np.random.default_rng(seed)
    dx, dy = 2 / (nx - 1), 2 / (ny - 1)
    p0 = 0.5 * rng.standard_normal((nx, ny))
    C = rng.standard_normal((nx, ny)) * dx * dy
    return (scale * p0).astype(dtype), (scale * C).astype(dtype), dx, dy


def oracle_solve(p0, C, dx, dy, beta, tol, max_sweeps):
    """The reference's loop (oracle.chorin_fd.get_pressure: `while err > tol and it < nit`, err = 1 before the first sweep) on a given C, in
    p0's type; dx, dy, beta are Python floats, which NumPy rounds to the arrays' type where they meet them.  Returns p, sweeps, last err."""
    T = p0.dtype.type
    p, prev, err, sweeps, tol = p0.copy(), p0.copy(), T(1), 0, T(tol)
    while err > tol and sweeps < max_sweeps:
        OC.sor_sweep_wavefront(p, C, dx, dy, beta)
        err = np.max(np.abs(p - prev))
        prev = p.copy()
        sweeps += 1
    assert p.dtype == p0.dtype and err.dtype == p0.dtype
    return p, sweeps, err


def _needs():
    need = {}
    for c in CASES:
        sw = need.setdefault((c.nx, c.ny, c.dtype, c.seed, c.scale), {0})
        sw.update(x for x in (c.stop, c.max_sweeps if c.stop is None else min(c.stop, c.max_sweeps)) if x is not None)
    for nx, ny, dt in BATCH_SHAPES:
        need.setdefault((nx, ny, dt, 0, 1.0), {0}).add(BATCH_STOP)
    return need


NEEDS = _needs()        # (nx, ny, dtype, seed, scale) -> the sweeps after which a case wants p or the error


@functools.lru_cache(maxsize=None)
def history(nx, ny, dtype, seed=0, scale=1.0):
    """The tolerance-free sweeps of a problem, computed once: errs[s - 1] = e_s up to the largest sweep a case needs, snaps[s] = p after s
    sweeps for the sweeps cases ask for (read-only; snaps[0] = p0)."""
    p0, C, dx, dy = problem(nx, ny, dtype, seed, scale)
    want = NEEDS[(nx, ny, dtype, seed, scale)]
    p, prev, errs, snaps = p0.copy(), p0.copy(), [], {0: p0}
    for s in range(1, max(want) + 1):
        OC.sor_sweep_wavefront(p, C, dx, dy, BETA)
        errs.append(np.max(np.abs(p - prev)))
        prev = p.copy()
        if s in want:
            snaps[s] = prev
    for a in snaps.values():
        a.setflags(write=False)
    assert p.dtype == np.dtype(dtype) and all(e.dtype == np.dtype(dtype) for e in errs)
    return errs, snaps


def tolerance(case):
    """tol of a case as the Python float handed to the library: e_s exactly (a float32 is a double), or 0."""
    return 0.0 if case.stop is None else float(history(case.nx, case.ny, case.dtype, case.seed, case.scale)[0][case.stop - 1])


def first_stop(case):
    """The first sweep whose error is <= the case's tol: 0 when the initial err = 1 already is, None for never."""
    return None if case.stop is None else 0 if tolerance(case) >= 1 else case.stop


def expected(case):
    """(sweeps, last err, p) of the reference's loop on a case: with a strictly decreasing history the loop under tol = e_s < 1 stops after
    sweep min(s, cap), under tol = e_s >= 1 before the first one, and under tol = 0 (never met while the errors stay positive) at the cap."""
    errs, snaps = history(case.nx, case.ny, case.dtype, case.seed, case.scale)
    n = case.max_sweeps if case.stop is None else min(first_stop(case), case.max_sweeps)
    return n, (errs[n - 1] if n else np.dtype(case.dtype).type(1)), snaps[n]


def bits(a):
    """The bit patterns of a float array or scalar (signed zeros and NaN payloads count)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
