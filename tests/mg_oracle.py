"""NumPy restatement (tests only) of the multigrid pressure-Poisson solver of csrc/mg_kernels.hip, and an exact discrete solver.

The equation is the fixed point of the reference's SOR update (src/chorin_fd/simulate.py:186-196): on interior points

    dy^2 (p[i+1,j] + p[i-1,j] - 2p) + dx^2 (p[i,j+1] + p[i,j-1] - 2p) = C[i,j],

with the boundary ring of p as Dirichlet data.  Every level works in the UNSCALED form  Lap_h u = f  with f = C * (1 / (dx^2 dy^2))
(cx = 1 / hx^2 along axis 0, cy = 1 / hy^2 along axis 1); the residual is r = f - Lap_h u.

Hierarchy: each axis coarsens on its own, n -> nc = (n - 1) // 2 + 1 nodes, spacing H = h (n - 1) / (nc - 1) (nested when n - 1 is even,
otherwise uniform coarse nodes on the same domain); coarsening stops once min(nx, ny) <= 9.  Refused (UnsupportedGrid): min(nx, ny) < 5, a
level whose cell aspect ratio exceeds 2, a coarsest level with more than 33 nodes on an axis.
Prolongation: per-axis linear interpolation by node coordinate; restriction R = (hx / Hx)(hy / Hy) P^T of the unscaled residual.
Smoother: red-black Gauss-Seidel, weight 1, colour 0 = (i + j) even.  V(2, 2): pre-smoothing colour 0 then 1, post-smoothing colour 1 then 0.
Coarsest level: exact solve of the error equation (sine-basis eigen-decomposition).
Stopping, per grid, after the cycle in which max|r_k| <= tol max|r_0| or max|r_k| >= 0.9 max|r_(k-1)|, or at max_cycles; max|r_0| = 0 or
non-finite runs no cycle.  Info: (cycles done, max|r_k| / max|r_0|); (0, 0) for a zero initial residual, (0, NaN) for a NaN or infinite one
(a NaN or Inf in C, in p's interior or in its boundary ring), (0, 1) for max_cycles = 0.

Launch split (host side of the solver, replayed by levels / tail_level / workspace_bytes): the levels from `tail` down to the coarsest run
in one workgroup's LDS, where tail is the finest level whose LDS (u and f of every level from there on, plus the coarsest solve's sine
tables and two work arrays) fits LDS_MAX bytes; the finer levels run chip-wide with u and f in the workspace.  The split is counted in
bytes, so one shape can take different paths in float32 and float64.

mutate= (vcycle, solve_one): a deliberately wrong variant of one operator, for the CPU tests that show a case's bounds would catch it:
  'post_order'      post-smoothing colours 0 then 1 (the solver: 1 then 0)
  'prolong_row'     the prolongation's row at fine node nx - 2 (axis 0) halved
  'restrict_scale'  restriction without the (hx / Hx)(hy / Hy) scale
  'coarse_mode'     the coarsest solve drops the highest sine mode of each axis (its mode loops one short)
"""
import numpy as np

MIN_N, STOP_N, MAX_ASPECT, MAX_COARSEST = 5, 9, 2.0, 33
MAX_LEV, LDS_MAX, INT_MAX = 16, 150 * 1024, 2**31 - 1
MUTATIONS = ('post_order', 'prolong_row', 'restrict_scale', 'coarse_mode')


class UnsupportedGrid(ValueError):
    pass


def hierarchy(nx, ny, dx, dy):
    """[(nx, ny, hx, hy)] from the finest level to the coarsest."""
    if min(nx, ny) < MIN_N:
        raise UnsupportedGrid("multigrid needs at least %d nodes per axis, got %d x %d" % (MIN_N, nx, ny))
    levs = [(nx, ny, float(dx), float(dy))]
    while True:
        n0, n1, h0, h1 = levs[-1]
        if max(h0 / h1, h1 / h0) > MAX_ASPECT:
            raise UnsupportedGrid("cell aspect ratio %.3g > %g at level %d" % (max(h0 / h1, h1 / h0), MAX_ASPECT, len(levs) - 1))
        if min(n0, n1) <= STOP_N:
            break
        c0, c1 = (n0 - 1) // 2 + 1, (n1 - 1) // 2 + 1
        levs.append((c0, c1, h0 * (n0 - 1) / (c0 - 1), h1 * (n1 - 1) / (c1 - 1)))
    if max(levs[-1][:2]) > MAX_COARSEST:
        raise UnsupportedGrid("coarsest level %d x %d exceeds %d nodes on an axis" % (levs[-1][0], levs[-1][1], MAX_COARSEST))
    return levs


# ---------------------------------------------------------------------------------------------------- the host-side launch split
def levels(nx, ny):
    """[(nx, ny)] of every level, finest first: mg_shape of csrc/mg_kernels.hip (no spacings, so no aspect check)."""
    if min(nx, ny) < MIN_N:
        raise UnsupportedGrid("multigrid needs at least %d nodes per axis, got %d x %d" % (MIN_N, nx, ny))
    if nx * ny > INT_MAX // 4:
        raise UnsupportedGrid("%d x %d grid too large" % (nx, ny))
    levs = [(nx, ny)]
    while min(levs[-1]) > STOP_N:
        if len(levs) == MAX_LEV:
            raise UnsupportedGrid("more than %d levels" % MAX_LEV)
        levs.append(((levs[-1][0] - 1) // 2 + 1, (levs[-1][1] - 1) // 2 + 1))
    if max(levs[-1]) > MAX_COARSEST:
        raise UnsupportedGrid("coarsest level %d x %d exceeds %d nodes on an axis" % (levs[-1][0], levs[-1][1], MAX_COARSEST))
    return levs


def tail_lds_elems(levs, l):
    """Elements of LDS of a tail that starts at level l (tail_lds_elems)."""
    mx, my = levs[-1][0] - 2, levs[-1][1] - 2
    return sum(2 * a * b for a, b in levs[l:]) + mx * mx + my * my + 2 * mx * my


def tail_level(nx, ny, elem_size):
    """The first level of the LDS tail (tail_level): 0 = the whole cycle in one workgroup."""
    levs = levels(nx, ny)
    l = len(levs) - 1
    while l > 0 and tail_lds_elems(levs, l - 1) * elem_size <= LDS_MAX:
        l -= 1
    return l


def tail_lds_bytes(nx, ny, elem_size):
    """Dynamic LDS of the tail launch, in bytes."""
    return tail_lds_elems(levels(nx, ny), tail_level(nx, ny, elem_size)) * elem_size


def _align256(x):
    return (x + 255) // 256 * 256


def workspace_bytes(B, nx, ny, elem_size, tail=None):
    """nns_fd_poisson_mg_workspace (mg_bytes): the per-grid state, then u and f of every chip-wide level 1 .. tail.  tail: the split to
    count for (default: the solver's, tail_level)."""
    levs = levels(nx, ny)
    t = tail_level(nx, ny, elem_size) if tail is None else tail
    return _align256(B * (4 + 4 + 8 + 8 + 8)) + sum(2 * _align256(B * a * b * elem_size) for a, b in levs[1:t + 1])


def prolongation(n, nc):
    """[n, nc]: fine node i at coarse coordinate s = i (nc - 1) / (n - 1); weights 1 - frac, frac on floor(s), floor(s) + 1."""
    P = np.zeros((n, nc))
    for i in range(n):
        num = i * (nc - 1)
        i0, rem = divmod(num, n - 1)
        frac = rem / (n - 1)
        if i0 >= nc - 1:
            P[i, nc - 1] = 1.0
        else:
            P[i, i0] = 1.0 - frac
            P[i, i0 + 1] = frac
    return P


def _coef(hx, hy):
    cx, cy = 1.0 / (hx * hx), 1.0 / (hy * hy)
    d = 2.0 * cx + 2.0 * cy
    return cx, cy, d, 1.0 / d


def residual(u, f, hx, hy):
    """r = f - Lap_h u on interior points, 0 on the boundary ring."""
    cx, cy, d, _ = _coef(hx, hy)
    r = np.zeros_like(u)
    r[1:-1, 1:-1] = f[1:-1, 1:-1] - (cx * (u[2:, 1:-1] + u[:-2, 1:-1]) + cy * (u[1:-1, 2:] + u[1:-1, :-2]) - d * u[1:-1, 1:-1])
    return r


def _colour_masks(nx, ny):
    i, j = np.meshgrid(np.arange(1, nx - 1), np.arange(1, ny - 1), indexing='ij')
    return ((i + j) % 2 == 0), ((i + j) % 2 == 1)


def half_sweep(u, f, hx, hy, mask):
    cx, cy, _, idg = _coef(hx, hy)
    nw = (cx * (u[2:, 1:-1] + u[:-2, 1:-1]) + cy * (u[1:-1, 2:] + u[1:-1, :-2]) - f[1:-1, 1:-1]) * idg
    inner = u[1:-1, 1:-1]
    inner[mask] = nw[mask]


def dst_solve(g, hx, hy, drop_top=False):
    """Exact solution of Lap_h e = g on the interior with e = 0 on the boundary ring (g: interior values [nx - 2, ny - 2]).
    drop_top: leave out the highest sine mode of each axis, every mode k = nx - 2 or l = ny - 2 (the 'coarse_mode' mutation)."""
    mx, my = g.shape
    nx, ny = mx + 2, my + 2
    kx, ky = np.arange(1, mx + 1), np.arange(1, my + 1)
    Sx = np.sin(np.pi * np.outer(kx, kx) / (nx - 1))
    Sy = np.sin(np.pi * np.outer(ky, ky) / (ny - 1))
    lx = -4.0 / (hx * hx) * np.sin(np.pi * kx / (2 * (nx - 1))) ** 2
    ly = -4.0 / (hy * hy) * np.sin(np.pi * ky / (2 * (ny - 1))) ** 2
    gh = Sx @ g @ Sy
    if drop_top:
        gh[-1, :] = gh[:, -1] = 0.0
    return (2.0 / (nx - 1)) * (2.0 / (ny - 1)) * (Sx @ (gh / (lx[:, None] + ly[None, :])) @ Sy)


def exact_solve(p, C, dx, dy):
    """The exact discrete solution of the pressure equation: p's boundary ring kept, the interior solved in float64."""
    p = np.array(p, dtype=np.float64)
    f = np.asarray(C, dtype=np.float64) * (1.0 / (dx * dx * dy * dy))
    g = residual(np.where(_ring(p.shape), p, 0.0), f, dx, dy)       # boundary data moved to the right-hand side
    p[1:-1, 1:-1] = dst_solve(g[1:-1, 1:-1], dx, dy)
    return p


def _ring(shape):
    m = np.zeros(shape, dtype=bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


def vcycle(levs, us, fs, l=0, mutate=None):
    assert mutate in (None,) + MUTATIONS, mutate
    nx, ny, hx, hy = levs[l]
    u, f = us[l], fs[l]
    if l == len(levs) - 1:
        r = residual(u, f, hx, hy)
        u[1:-1, 1:-1] += dst_solve(r[1:-1, 1:-1], hx, hy, drop_top=mutate == 'coarse_mode')
        return
    c0, c1 = _colour_masks(nx, ny)
    for _ in range(2):
        half_sweep(u, f, hx, hy, c0)
        half_sweep(u, f, hx, hy, c1)
    ncx, ncy, Hx, Hy = levs[l + 1]
    Px, Py = prolongation(nx, ncx), prolongation(ny, ncy)
    r = residual(u, f, hx, hy)
    fc = np.zeros((ncx, ncy))
    sxy = 1.0 if mutate == 'restrict_scale' else (hx / Hx) * (hy / Hy)
    fc[1:-1, 1:-1] = (sxy * (Px.T @ r @ Py))[1:-1, 1:-1]
    fs[l + 1] = fc
    us[l + 1] = np.zeros((ncx, ncy))
    vcycle(levs, us, fs, l + 1, mutate)
    if mutate == 'prolong_row':
        Px = Px.copy()
        Px[nx - 2] *= 0.5
    u[1:-1, 1:-1] += (Px @ us[l + 1] @ Py.T)[1:-1, 1:-1]
    post = (c0, c1) if mutate == 'post_order' else (c1, c0)
    for _ in range(2):
        half_sweep(u, f, hx, hy, post[0])
        half_sweep(u, f, hx, hy, post[1])


def solve_one(p, C, dx, dy, tol=1e-6, max_cycles=30, mutate=None):
    """One grid.  Returns (p after the solve, info (cycles, ratio), [max|r_k| for k = 0 .. cycles])."""
    levs = hierarchy(p.shape[0], p.shape[1], dx, dy)
    u = np.array(p, dtype=np.float64)
    f = np.asarray(C, dtype=np.float64) * (1.0 / (dx * dx * dy * dy))
    with np.errstate(invalid='ignore', over='ignore'):
        rn = [float(np.max(np.abs(residual(u, f, dx, dy))))]     # NaN if any residual is NaN (np.max propagates it)
    if not np.isfinite(rn[0]):
        return u, (0, float('nan')), rn
    if rn[0] == 0:
        return u, (0, 0.0), rn
    if max_cycles <= 0:
        return u, (0, 1.0), rn
    us, fs = [u] + [None] * (len(levs) - 1), [f] + [None] * (len(levs) - 1)
    k = 0
    while k < max_cycles:
        vcycle(levs, us, fs, mutate=mutate)
        k += 1
        rn.append(float(np.max(np.abs(residual(u, f, dx, dy)))))
        if not (rn[k] > tol * rn[0] and rn[k] < 0.9 * rn[k - 1]):
            break
    return u, (k, rn[k] / rn[0]), rn


def solve(p, C, dx, dy, tol=1e-6, max_cycles=30):
    """p, C: [nx, ny] or [B, nx, ny].  Returns (p, info [B, 2])."""
    p3, C3 = np.asarray(p), np.asarray(C)
    one = p3.ndim == 2
    if one:
        p3, C3 = p3[None], C3[None]
    outs, infos = [], []
    for b in range(p3.shape[0]):
        u, inf, _ = solve_one(p3[b], C3[b], dx, dy, tol, max_cycles)
        outs.append(u), infos.append(inf)
    out = np.stack(outs)
    return (out[0] if one else out), np.array(infos, dtype=np.float64)


def random_problem(nx, ny, seed=0, B=None):
    """A random boundary ring, a zero interior and a random right-hand side (C in the solver's scaled form)."""
    rng = np.random.default_rng(seed)
    shape = (nx, ny) if B is None else (B, nx, ny)
    p = rng.standard_normal(shape)
    p[..., 1:-1, 1:-1] = 0.0
    C = rng.standard_normal(shape)
    C[..., 0, :] = C[..., -1, :] = C[..., :, 0] = C[..., :, -1] = 0.0
    return p, C


def spacings(nx, ny):
    """The chorin_fd spacings: a [-1, 1]^2 box (src/chorin_fd/simulate.py:58)."""
    return 2.0 / (nx - 1), 2.0 / (ny - 1)
