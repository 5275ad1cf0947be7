"""CPU checks of the multigrid restatement (tests/mg_oracle.py) that the GPU solver (csrc/mg_kernels.hip) is compared against: its exact
discrete solver, its hierarchy, its convergence per cycle, the grids it refuses, its replica of the host's launch split, the edge cases of
tests/mg_cases.py and how far a wrong operator would move them."""
import json
import os

import numpy as np
import pytest

import mg_cases as K
import mg_oracle as M
from conftest import ROOT, rel_l2

SIZES = [(33, 33), (50, 50), (51, 51), (64, 64), (64, 50), (96, 96), (129, 129), (200, 200), (1024, 1024)]


def _assembled_solve(p, C, dx, dy):
    """numpy.linalg.solve of the assembled 5-point system (scaled form, boundary data moved to the right-hand side)."""
    nx, ny = p.shape
    mx, my = nx - 2, ny - 2
    idx = lambda i, j: (i - 1) * my + (j - 1)
    A = np.zeros((mx * my, mx * my))
    rhs = np.zeros(mx * my)
    for i in range(1, nx - 1):
        for j in range(1, ny - 1):
            r = idx(i, j)
            A[r, r] = -(2 * dy * dy + 2 * dx * dx)
            rhs[r] = C[i, j]
            for (a, b, w) in ((i + 1, j, dy * dy), (i - 1, j, dy * dy), (i, j + 1, dx * dx), (i, j - 1, dx * dx)):
                if 0 < a < nx - 1 and 0 < b < ny - 1:
                    A[r, idx(a, b)] = w
                else:
                    rhs[r] -= w * p[a, b]
    out = p.copy()
    out[1:-1, 1:-1] = np.linalg.solve(A, rhs).reshape(mx, my)
    return out


def test_exact_solver_matches_dense_solve():
    nx, ny = 12, 9
    dx, dy = M.spacings(nx, ny)
    p, C = M.random_problem(nx, ny, seed=3)
    ref = _assembled_solve(p, C, dx, dy)
    got = M.exact_solve(p, C, dx, dy)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-12
    assert np.array_equal(got[0], p[0]) and np.array_equal(got[:, -1], p[:, -1])


def test_hierarchy_matches_the_issue_table():
    lv = lambda nx, ny: [l[:2] for l in M.hierarchy(nx, ny, *M.spacings(nx, ny))]
    assert lv(50, 50) == [(50, 50), (25, 25), (13, 13), (7, 7)]
    assert lv(64, 50) == [(64, 50), (32, 25), (16, 13), (8, 7)]
    assert [a for a, _ in lv(1024, 1024)] == [1024, 512, 256, 128, 64, 32, 16, 8]
    h = M.hierarchy(50, 50, *M.spacings(50, 50))
    for (n, _, hx, _), (nc, _, Hx, _) in zip(h, h[1:]):
        assert abs(hx * (n - 1) - Hx * (nc - 1)) < 1e-14            # same domain at every level


def test_prolongation_is_linear_interpolation():
    for n in (50, 51, 64):
        nc = (n - 1) // 2 + 1
        P = M.prolongation(n, nc)
        assert np.allclose(P.sum(axis=1), 1.0)
        X = np.arange(nc) / (nc - 1)
        assert np.allclose(P @ X, np.arange(n) / (n - 1))             # exact on linear functions of the node coordinate


@pytest.mark.parametrize('nx,ny', SIZES)
def test_convergence_per_cycle(nx, ny):
    dx, dy = M.spacings(nx, ny)
    p, C = M.random_problem(nx, ny, seed=nx + ny)
    u, (cycles, ratio), rn = M.solve_one(p, C, dx, dy, tol=1e-10, max_cycles=30)
    rates = np.array(rn[1:]) / np.array(rn[:-1])
    assert np.median(rates) <= 0.2, rates
    assert cycles <= 14 and ratio <= 1e-10, (cycles, ratio)
    assert np.array_equal(u[0], p[0]) and np.array_equal(u[-1], p[-1]) and np.array_equal(u[:, 0], p[:, 0]) and np.array_equal(u[:, -1], p[:, -1])
    if nx * ny <= 200 * 200:
        ex = M.exact_solve(p, C, dx, dy)
        assert np.linalg.norm(u - ex) / np.linalg.norm(ex) < 1e-8


def test_stopping_rule_and_info():
    dx, dy = M.spacings(50, 50)
    p, C = M.random_problem(50, 50, seed=1)
    _, (cycles, ratio), rn = M.solve_one(p, C, dx, dy, tol=1e-6, max_cycles=30)
    assert rn[cycles] <= 1e-6 * rn[0] and rn[cycles - 1] > 1e-6 * rn[0] and ratio == rn[cycles] / rn[0]
    _, (c3, _), _ = M.solve_one(p, C, dx, dy, tol=0.0, max_cycles=3)
    assert c3 == 3
    # a zero residual: no cycle, p unchanged
    z = np.full_like(p, 0.25)
    C0 = np.zeros_like(C)
    u, info, _ = M.solve_one(z, C0, dx, dy)
    assert info == (0, 0.0) and np.array_equal(u, z)
    # float64 rounding floor: tol = 0 ends on the stagnation rule before max_cycles
    _, (cs, _), rn = M.solve_one(p, C, dx, dy, tol=0.0, max_cycles=60)
    assert cs < 60 and rn[cs] >= 0.9 * rn[cs - 1]


def test_unsupported_grids_are_refused():
    with pytest.raises(M.UnsupportedGrid):
        M.hierarchy(4, 64, 0.1, 0.1)
    with pytest.raises(M.UnsupportedGrid):
        M.hierarchy(64, 64, 1.0, 0.3)                                  # aspect ratio 3.3 at the finest level
    with pytest.raises(M.UnsupportedGrid):
        M.hierarchy(1024, 64, 0.01, 0.01)                              # coarsest 128 x 8
    M.hierarchy(9, 9, 0.25, 0.25)                                      # one level: the exact solve alone


# ---------------------------------------------------------------------------------------------------- the launch split and the edge cases
def test_split_replica_matches_the_recorded_run():
    """tail_level as profiles/mg_run.json recorded it from the library on the MI355X, in both types."""
    with open(os.path.join(ROOT, 'profiles', 'mg_run.json')) as fh:
        run = json.load(fh)
    seen = set()
    for c in run['cases']:
        elem = 4 if c['dtype'] == 'f32' else 8
        assert [list(l) for l in M.levels(c['n'], c['n'])] == c['levels']
        assert M.tail_level(c['n'], c['n'], elem) == c['tail_level'], c
        seen.add((c['n'], elem, c['tail_level']))
    assert {(64, 4, 0), (64, 8, 0), (512, 4, 3), (512, 8, 3), (1024, 4, 4), (1024, 8, 4)} <= seen


def test_split_replica_finds_the_lds_limits():
    for n, t32, t64 in ((84, 0, 0), (85, 0, 1), (119, 0, 1), (120, 1, 1), (128, 1, 1), (200, 1, 2)):
        assert (M.tail_level(n, n, 4), M.tail_level(n, n, 8)) == (t32, t64), n
    whole = lambda n, elem: M.tail_lds_elems(M.levels(n, n), 0) * elem              # the whole cycle in LDS
    assert whole(84, 8) <= M.LDS_MAX < whole(85, 8) and whole(119, 4) <= M.LDS_MAX < whole(120, 4)
    assert '%.1f %.1f' % (whole(84, 8) / 1024, whole(119, 4) / 1024) == '147.7 148.6'
    assert M.workspace_bytes(3, 84, 84, 8) == 256 < M.workspace_bytes(3, 85, 85, 8)   # tail 0: the per-grid state only


def test_case_matrix_covers_every_path_and_is_supported():
    paths = set()
    for c, why in K.CASES:
        nx, ny, B, dx, dy = c
        levs = M.hierarchy(nx, ny, dx, dy)
        aspect = max(max(h0 / h1, h1 / h0) for _, _, h0, h1 in levs)
        p32, p64 = K.path(nx, ny, 4), K.path(nx, ny, 8)
        print('%-22s levels %d  coarsest %2dx%-2d  aspect <= %.3f  f32 %-6s tail %d  f64 %-6s tail %d  (%s)' % (
            K.case_id(c), len(levs), levs[-1][0], levs[-1][1], aspect, p32, M.tail_level(nx, ny, 4), p64, M.tail_level(nx, ny, 8), why))
        paths |= {(p32, 4), (p64, 8)}
    assert paths == {(p, e) for p in ('single', 'lds', 'mixed') for e in (4, 8)}
    assert max(max(c[:2]) for c, _ in K.CASES if K.path(c[0], c[1], 8) == 'single') == 33          # a 33-node coarsest axis
    for nx, ny, dx, dy, refused in K.SHAPE_CHECKS:
        try:
            M.hierarchy(nx, ny, dx, dy)
            got = False
        except M.UnsupportedGrid as e:
            got = True
            print('%dx%d dx/dy %.4g refused: %s' % (nx, ny, dx / dy, e))
        assert got == refused, (nx, ny, dx / dy)


@pytest.mark.parametrize('case', [c for c, _ in K.CASES], ids=[K.case_id(c) for c, _ in K.CASES])
def test_mutations_move_one_cycle_past_the_f32_bound(case):
    # each deliberately wrong operator moves p after one cycle by >= 10x the case's float32 bound for k = 1 (the float64 bound is 1e-11), so
    # the GPU comparison would catch it in either type.  On one level only the coarsest solve runs, so only 'coarse_mode' applies there.
    # Measured here: post_order 2.7e-2 .. 6.0e-2, prolong_row 1.8e-3 .. 3.2e-2, restrict_scale 2.0 .. 1.4e4, coarse_mode 8.1e-5 .. 1.2e-2
    # (single level 7.2e-2 .. 0.27): at least 54x the bound.
    nx, ny, B, dx, dy = case
    P, Cs = K.problem(case)
    base, _, _ = M.solve_one(P[0], Cs[0], dx, dy, tol=0.0, max_cycles=1)
    bound = K.BOUND_F32[K.path(nx, ny, 4), 1]
    muts = M.MUTATIONS if K.path(nx, ny, 8) != 'single' else ('coarse_mode',)
    moves = {m: rel_l2(M.solve_one(P[0], Cs[0], dx, dy, tol=0.0, max_cycles=1, mutate=m)[0], base) for m in muts}
    print('%s (f32 bound %.1e): %s' % (K.case_id(case), bound, '  '.join('%s %.1e' % kv for kv in moves.items())))
    for m, d in moves.items():
        assert d >= 10 * bound, (m, d, bound)


def test_non_finite_data_is_never_a_zero_residual():
    nx = ny = 33
    dx, dy = M.spacings(nx, ny)
    p, C = M.random_problem(nx, ny, seed=6)
    for name, (a, idx, val) in {'NaN in C': ('C', (16, 9), np.nan), 'Inf in C': ('C', (3, 4), np.inf),
                                'NaN in the ring': ('p', (0, 7), np.nan), '-Inf inside': ('p', (20, 20), -np.inf)}.items():
        pp, CC = p.copy(), C.copy()
        (pp if a == 'p' else CC)[idx] = val
        u, info, rn = M.solve_one(pp, CC, dx, dy)
        assert info[0] == 0 and np.isnan(info[1]) and not np.isfinite(rn[0]), name
        assert np.array_equal(u, pp, equal_nan=True), name
    u, info, _ = M.solve_one(np.full_like(p, 0.25), np.zeros_like(C), dx, dy)       # a zero residual is still (0, 0)
    assert info == (0, 0.0)
