"""The lexicographic SOR solve (nns_fd_sor_*, csrc/sor_device.h) BITWISE against the reference's loop (oracle/chorin_fd.py) on every pipeline
(one lane per row, fronts in LDS, fronts in global memory), in float64 and float32: non-square grids, one interior row / column / point,
exactly 64 interior rows, the LDS boundaries, and the stop on the first, an inner and the last sweep of every kind of speculative batch, on
err == tol exactly, on a batch the sweep cap cut short, under every kind of hint; batches of grids that stop at different sweeps; tolerances
at or above the initial err = 1 (no sweep at all), zeros, signed zeros and a NaN.  Then the fused explicit step (nns_fd_step_explicit_*),
which runs the same solve, against the separate operators on non-square grids.  The cases are in tests/sor_cases.py; tests/test_oracle_sor.py
shows on the CPU that they are what they say.

The kernels keep the reference's operation order (no FMA contraction), their maximum is exact and div_den is bitwise the division, so the
sweep count, the last error and every value of p are compared as bit patterns in both types; no tolerance is involved."""
import numpy as np
import pytest
import torch

import sor_cases as K
from conftest import rel_l2

pytestmark = pytest.mark.gpu

GROUPS = sorted({(c.nx, c.ny, c.dtype) for c in K.CASES})
TORCH = {K.F64: torch.float64, K.F32: torch.float32}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def solve(p0, C, dx, dy, tol, max_sweeps, hint=None):
    """ops.fd_sor_ on copies of host arrays ([nx, ny] or [B, nx, ny]); hint: a sweep count for every grid.  Returns p and info [B, 2]."""
    from nns import ops
    p = dev(p0)
    B = 1 if p.dim() == 2 else p.shape[0]
    h = None if hint is None else torch.tensor([[hint, 0.0]] * B, dtype=p.dtype, device='cuda')
    info = ops.fd_sor_(p, dev(C), dx, dy, K.BETA, tol, max_sweeps, hint=h)
    return p.cpu().numpy(), info.cpu().numpy()


def mismatch(p, info, ref_p, ref_sweeps, ref_err):
    """What differs between one grid's result and the oracle's, as text ('' when nothing does): bit patterns, a NaN equals a NaN."""
    out = []
    if int(info[0]) != ref_sweeps:
        out.append('sweeps %d != %d' % (int(info[0]), ref_sweeps))
    if not (K.bits(info[1]) == K.bits(ref_err) or (np.isnan(info[1]) and np.isnan(ref_err))):
        out.append('err %r != %r' % (info[1], ref_err))
    if p.dtype != ref_p.dtype or p.shape != ref_p.shape:
        out.append('p is %s %s' % (p.dtype, p.shape))
    elif np.isnan(ref_p).any():
        if not np.array_equal(p, ref_p, equal_nan=True):
            out.append('p differs (NaN pattern or values)')
    elif K.bits(p).tobytes() != K.bits(ref_p).tobytes():
        bad = np.argwhere(K.bits(p) != K.bits(ref_p))
        out.append('p differs at %d points, first %s: %r != %r' % (len(bad), tuple(bad[0]), p[tuple(bad[0])], ref_p[tuple(bad[0])]))
    return ', '.join(out)


def test_lds_fit_is_the_librarys_own_predicate(gpu_device):
    """The pipeline a case is said to take rests on the restated LDS arithmetic: the library's predicate agrees on every shape, either type."""
    from nns import ops
    shapes = {(s[0], s[1]) for s in K.SHAPES} | {(s[0], s[1]) for s in K.FUSED} | {(s[0], s[1]) for s in K.SPECIAL_SHAPES + K.BATCH_SHAPES}
    for nx, ny in sorted(shapes):
        for dt in (K.F64, K.F32):
            assert ops.fd_step_explicit_fits(nx, ny, TORCH[dt]) == K.fits_lds(nx, ny, dt), (nx, ny, dt)


@pytest.mark.parametrize('group', GROUPS, ids=[K.shape_id(*g) for g in GROUPS])
def test_solve_is_bitwise_the_oracle(group, gpu_device):
    """Every stop, cap and hint case of one shape and type: sweep count, last error and p as bit patterns."""
    cases = [c for c in K.CASES if (c.nx, c.ny, c.dtype) == group]
    failures = []
    for c in cases:
        p0, C, dx, dy = K.problem(c.nx, c.ny, c.dtype, c.seed, c.scale)
        sweeps, err, ref = K.expected(c)
        p, info = solve(p0, C, dx, dy, K.tolerance(c), c.max_sweeps, hint=c.hint or None)
        bad = mismatch(p, info[0], ref, sweeps, err)
        if bad:
            failures.append('%s stop=%s cap=%d hint=%d scale=%g tol=%r (oracle: %d sweeps; plan %s): %s' % (
                c.kind, c.stop, c.max_sweeps, c.hint, c.scale, K.tolerance(c), sweeps, c.plan.batches, bad))
    assert not failures, '%d of %d cases of %s (%s)\n' % (len(failures), len(cases), K.shape_id(*group), cases[0].pipeline) + '\n'.join(failures)


@pytest.mark.parametrize('dtype', [K.F64, K.F32])
def test_one_interior_point_under_zero_tolerance(dtype, gpu_device):
    """3 x 3: the error reaches 0 exactly, and `0 > 0` ends the loop where the oracle says (sweep 29 / 15)."""
    p0, C, dx, dy = K.problem(3, 3, dtype)
    ref, sweeps, err = K.oracle_solve(p0, C, dx, dy, K.BETA, 0.0, K.MANY)
    p, info = solve(p0, C, dx, dy, 0.0, K.MANY)
    assert 1 < sweeps < K.MANY and not mismatch(p, info[0], ref, sweeps, err), mismatch(p, info[0], ref, sweeps, err)


@pytest.mark.parametrize('shape', K.BATCH_SHAPES, ids=[K.shape_id(*s) for s in K.BATCH_SHAPES])
def test_batch_of_grids_that_stop_at_different_sweeps(shape, gpu_device):
    """Three grids in one launch (one workgroup each), one C, p0 scaled by 1, 1e-3, 1e3, one tolerance: the oracle runs per grid."""
    nx, ny, dt = shape
    p0, C, dx, dy = K.problem(nx, ny, dt)
    T = np.dtype(dt).type
    tol = float(K.history(nx, ny, dt)[0][K.BATCH_STOP - 1])
    P0 = np.stack([p0 * T(s) for s in K.BATCH_SCALES])
    p, info = solve(P0, np.stack([C] * 3), dx, dy, tol, K.BATCH_CAP)
    for b in range(3):
        ref, sweeps, err = K.oracle_solve(P0[b], C, dx, dy, K.BETA, tol, K.BATCH_CAP)
        bad = mismatch(p[b], info[b], ref, sweeps, err)
        assert not bad, (b, sweeps, bad)


@pytest.mark.parametrize('shape', K.SPECIAL_SHAPES, ids=[K.shape_id(*s) for s in K.SPECIAL_SHAPES])
def test_special_values(shape, gpu_device):
    """tol >= the initial err = 1: the reference's `while err > tol` runs no sweep, info = (0, 1), p untouched.  All zeros under tol = 0: one
    sweep, whose error 0 is not > 0; zeros of either sign in C and in p0.  One NaN in C: the loop stops after the sweep that makes err NaN."""
    nx, ny, dt = shape
    p0, C, dx, dy = K.problem(nx, ny, dt)
    T = np.dtype(dt).type
    z = np.zeros_like(p0)
    Cneg = z.copy()
    Cneg[1::2, ::3] = -0.0
    Cnan = C.copy()
    Cnan[nx // 2, ny // 2] = np.nan
    failures = []
    for what, a, c, tol, cap, hint in (('tol 2', p0, C, 2.0, 40, None), ('tol 1', p0, C, 1.0, 40, None), ('tol 1, hint 5', p0, C, 1.0, 40, 5),
                                       ('tol 2, zeros', z, z, 2.0, 40, None),
                                       ('zeros', z, z, 0.0, 40, None), ('C of -0.0', z, Cneg, 0.0, 40, None), ('p0 of -0.0', -z, z, 0.0, 40, None),
                                       ('p0 of -0.0, C of -0.0', -z, Cneg, 0.0, 40, None), ('NaN in C', p0, Cnan, 1e-3, 40, None)):
        ref, sweeps, err = K.oracle_solve(a, c, dx, dy, K.BETA, tol, cap)
        if what.startswith('tol'):
            assert sweeps == 0 and err == T(1) and ref.tobytes() == a.tobytes()
        elif what == 'NaN in C':
            assert sweeps == 1 and np.isnan(err) and np.isnan(ref).sum() > 1
        else:
            assert sweeps == 1 and err == 0 and not ref.any()
        p, info = solve(a, c, dx, dy, tol, cap, hint=hint)
        bad = mismatch(p, info[0], ref, sweeps, err)
        if bad:
            failures.append('%s: %s' % (what, bad))
    assert not failures, '%s (%s)\n' % (K.shape_id(*shape), K.pipeline(nx, ny, dt)) + '\n'.join(failures)


# ---------------------------------------------------------------------------------------------------- the fused explicit step
STEP = dict(dt=1e-3, rho=1.1, nu=0.02)
# tol and cap of the six-step runs: under them the solves of these grids stop between sweeps 12 and 68, a different one every step
STEP_TOL, STEP_CAP = 3e-2, 120


def step_fields(nx, ny, dtype):
    rng = np.random.default_rng(nx * 1000 + ny)
    return [(0.05 * rng.standard_normal((nx, ny))).astype(dtype) for _ in range(5)]        # u, v, u1, v1, p


def step_fused(f, bls, dx, dy, tol, cap, corrected, hint):
    from nns import ops
    u, v, u1, v1, p = f
    un, vn, info = ops.fd_step_explicit(u, v, u1, v1, p, bls[0], bls[1], bls[2], STEP['dt'], dx, dy, STEP['rho'], STEP['nu'], K.BETA, tol, cap,
                                        corrected=corrected, hint=hint)
    return [un, vn, u, v, p], info


def step_separate(f, bls, dx, dy, tol, cap, corrected, hint):
    """The sequence the fused step replaces, in its order."""
    from nns import ops
    u, v, u1, v1, p = f
    pred = ops.fd_predictor_explicit_corrected if corrected else ops.fd_predictor_explicit
    ui, vi = pred(u, v, u1, v1, STEP['dt'], dx, dy, STEP['nu'])
    ops.bc_apply_(ui, bls[0])
    ops.bc_apply_(vi, bls[1])
    C = ops.fd_pressure_rhs(ui, vi, STEP['dt'], dx, dy, STEP['rho'])
    info = ops.fd_sor_(p, C, dx, dy, K.BETA, tol, cap, hint=hint)
    ops.bc_apply_(p, bls[2])
    un, vn = ops.fd_correction(ui, vi, p, STEP['dt'], dx, dy)
    return [un, vn, u, v, p], info


@pytest.mark.parametrize('case', K.FUSED, ids=[K.shape_id(*c[:3]) + ('-corrected' if c[3] else '') for c in K.FUSED])
def test_fused_explicit_step_on_non_square_grids(case, gpu_device):
    """Six steps of a lid-driven start from small random fields, each solve hinted with the previous step's info: u, v, p and info of the one
    launch are bitwise those of the seven.  The first (40, 56) step against oracle.chorin_fd.step; tol = 2 leaves p at its boundary-list image."""
    from nns import ops
    from oracle import chorin_fd as OC
    from oracle.boundary import cavity_bcs, apply_bc_list
    nx, ny, dtype, corrected, _ = case
    dx, dy = 2 / (nx - 1), 2 / (ny - 1)
    bcs = cavity_bcs(dx, dy)
    bls = [ops.make_bc_list(b) for b in bcs]
    assert ops.fd_step_explicit_fits(nx, ny, TORCH[dtype])
    host = step_fields(nx, ny, dtype)
    runs = []
    for step in (step_fused, step_separate):
        f, info, trace = [dev(a) for a in host], None, []
        for _ in range(6):
            f, info = step(f, bls, dx, dy, STEP_TOL, STEP_CAP, corrected, info)
            trace.append([t.clone() for t in (f[0], f[1], f[4], info)])
        runs.append(trace)
    for k, (a, b) in enumerate(zip(*runs)):
        for name, x, y in zip(('u', 'v', 'p', 'info'), a, b):
            assert K.bits(x.cpu().numpy()).tobytes() == K.bits(y.cpu().numpy()).tobytes(), (k, name, a[3].cpu().numpy(), b[3].cpu().numpy())
    sweeps = [int(t[3][0, 0]) for t in runs[0]]
    assert len(set(sweeps)) > 1 and 0 < min(sweeps) and max(sweeps) < STEP_CAP, sweeps        # early stops, hints that are off
    assert float(runs[0][-1][0].abs().max()) == 1.0                                             # the lid
    # tol >= the initial err = 1: no sweep, p is the boundary-list image of what came in (the oracle's list, bitwise the kernel's)
    for step in (step_fused, step_separate):
        f, info = step([dev(a) for a in host], bls, dx, dy, 2.0, STEP_CAP, corrected, None)
        info = info.cpu().numpy()
        assert int(info[0, 0]) == 0 and info[0, 1] == 1, (step.__name__, info)
        assert K.bits(f[4].cpu().numpy()).tobytes() == K.bits(apply_bc_list(host[4].copy(), bcs[2])).tobytes(), step.__name__
    if (nx, ny) == (40, 56):
        nit = 50
        ur, vr, pr, (n, err) = OC.step(*[a.copy() for a in host], *bcs, STEP['dt'], dx, dy, STEP['rho'], STEP['nu'], K.BETA, nit, method='explicit',
                                      return_info=True)
        f, info = step_fused([dev(a) for a in host], bls, dx, dy, OC.SOR_TOL, nit - 1, corrected, None)
        assert int(info[0, 0]) == n
        for got, ref in zip((f[0], f[1], f[4]), (ur, vr, pr)):
            assert rel_l2(got.cpu().numpy(), ref) <= 1e-12
