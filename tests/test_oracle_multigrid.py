"""CPU checks of the multigrid restatement (tests/mg_oracle.py) that the GPU solver (csrc/mg_kernels.hip) is compared against: its exact
discrete solver, its hierarchy, its convergence per cycle and the grids it refuses."""
import numpy as np
import pytest

import mg_oracle as M

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
