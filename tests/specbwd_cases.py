"""Cases of the spectral residual backward, nns_spec_residual_bwd_f32 (csrc/spectral_bwd_kernels.hip; tests/test_gpu_specbwd.py runs them on the
GPU, tests/test_oracle_specbwd.py runs every condition on the reference alone, without one).  No GPU code here.

Dispatch (csrc/spectral_bwd_kernels.hip, csrc/spectral_common.h), restated in `dispatch`:
  per axis   a power of two in [64, 1024] goes through the FFT engine, any other length through the float64 circulant form (spectral_dense.hip);
  arithmetic amplification(axis) = nu pi N / (sqrt(3) L).  precise = 0: float32 transforms; 2: float64 forward transforms; 1: float32 while the
             amplification is <= 8 (kF32AmpMax).  ONE decision for both passes (spec_resolve_precise): float32 only if every FFT axis allows it;
  x-pass     a tile is LINES = 8192 / nx columns of one grid, ceil(ny / LINES) tiles per grid, min(tiles, 512) workgroups stride over them
             (spec_grid_cap).  float32: spec_bwd_xsplit_kernel, memory waves and transform waves; float64: spec_bwd_xpass_kernel<N, double>;
  y-pass     a row group is LINES = 8192 / ny rows of the batch * nx rows, min(groups, 512) workgroups stride over them: spec_bwd_ypass_kernel.
spec_bwd_xpass_kernel exists for float64 forward transforms only: launch_bwd_xpass hands every float32 x-pass to the role-split kernel, whose
32-bit byte offsets need N * ny < 2^30, and ny <= 2048 (kDenseMaxLen) keeps N * ny <= 2^21 through the C ABI (beyond: NNS_ERR_UNSUPPORTED).

Inputs: grid b of an nx x ny case is five fields (u, v, g_u, g_v, g_div) from one torch.Generator seeded from (nx, ny, b): white noise (N(0, 1), drawn in
float32), its rfft2 multiplied by (1 + |m|)^-1 (m the integer wavenumber vector), transformed back, scaled to max-abs 1, cast to float32 -- energy up to and
including both Nyquist lines.  dt = 1 (g / dt does not set the scale), rho = 1.3, Lx = 1.5, Ly = 4.0 (exchanged in the cases marked swap), and
nu = A sqrt(3) L / (pi N) on the axis with the largest N / L: A is that axis' amplification.  A in {0.1, 4} where float32 transforms are
legitimate, A = 20 where only float64 ones are.

Bounds, per output (grad_u, grad_v, grad_p), rel-L2 against the float64 oracle (oracle/periodic.py: spectral_residual_vjp):
  precise = 0   1e-5, the project's north-star bar (BASELINE.json) and the one the forward's float32 mode is held to; only cases with A <= 8;
  precise = 2   min(1e-5, max(10 * e32, 1e-6)): e32 is the largest rel-L2 between the oracle's formula evaluated in float32 (`vjp`, torch CPU
                rfft2 in float32) and in float64 -- the kernel's three inverse transforms are float32 too; 10 is a margin, 1e-6 the bar the
                forward's precise = 2 and the dense backward already meet.
  grad_u_prev, grad_v_prev   bitwise -(g * float32(1 / dt)).
Nothing is measured from the kernels.  Eight deliberately wrong float64 oracles (`vjp(..., mutation=)`, MUTATIONS) miss the bound of every case
they apply to by >= 100 x in at least one output (test_oracle_specbwd.py).  The Nyquist one has the form the kernels could get wrong: the odd
derivative of a packed pair f + i g by a complex FFT with the Nyquist wavenumber kept, which adds -k_N G_N (-1)^j to f' and +k_N F_N (-1)^j
to g' for the pairs (u, v), (g_u, g_v), (s1, s2) of the kernel's header comment.

The multi-tile cases (MULTI): `ntiles > 2 * 512, ntiles % 512 != 0, some workgroup gets >= 3 tiles` holds for the pass each is there for, except
(600, 7, 1024), whose 4200 rows make 525 float64 row groups of 8: a second iteration for 13 workgroups, but 4200 = 525 * 8 leaves the last
group full, so (601, 7, 1024) stands next to it: 526 groups, the last with 7 rows, in a second iteration.  The float64 row kernel's three-deep loop
is reached by the y-pass of (140, 1024, 64) at precise = 2 (1120 row groups).

Measured on an MI355X: the worst rel-L2 against the float64 oracle over all cases and outputs that run a path, and the path's smallest margin
bound / error (a case runs two paths; its figures count for both).  On the reference alone e32 is 2.4e-7 .. 1.7e-6 over all cases, and the
wrong oracle that moves least is `drop_pointwise` at (3, 7, 1024), A = 20: 3.3e-3, 330 x the bound.
  path                worst error                               smallest margin
  float32 x-split     3.1e-7  grad_v  B2-512x100-p0-A0.1        32 x  (the same, of 1e-5)
  float32 y           3.0e-7  grad_u  B3-7x1024-p0-A0.1         33 x  (the same, of 1e-5)
  float64 x           2.3e-7  grad_v  B2-1024x100-p2-A0.1       21 x  grad_v  B1-256x256-p2-A0.1  (1.6e-7 of 3.4e-6)
  float64 y           2.7e-7  grad_u  B3-7x1024-p2-A0.1         21 x  (the same case)
  dense-mixed         3.1e-7  grad_v  B2-512x100-p0-A0.1        22 x  grad_v  B2-256x100-p2-A0.1  (1.7e-7 of 3.9e-6)
  multi-tile calls    1.8e-7  grad_v  B140-1024x64-p0-A4        55 x  (the same, of 1e-5); all six equal their pieces bitwise
The float32 mode is no worse at A = 4 (at most 1.8e-7) than at A = 0.1.  The Nyquist mode: grad_p exactly 0 and grad_u within 2e-8 of
(1 / dt + nu k_N^2) g_u in all eight cases; the leak probe within 5.2e-7 of the oracle.  Nothing exceeded its bound; nothing in the kernels
was changed.

What the tests reject, run once against deliberately wrong builds of csrc/spectral_bwd_kernels.hip (arithmetic changes only, each in bounds,
none kept):
  (a) the memory waves of spec_bwd_xsplit_kernel never put the next tile's u, v, g_u into the exchange image (`has_next` taken as false
      there only) -> the bitwise comparison of the three float32 multi-tile cases fails, at the first piece, and nothing else does: every
      other test gives each workgroup one tile;
  (b) the sign of c2 flipped where adj_core forms -nu k^2 Z2 in float64 -> every precise = 2 case fails (45 of test_backward_vs_oracle, the
      three float64 multi-tile cases, the four precise = 2 Nyquist cases, the precise = 2 autograd case, and the oracle comparison of the
      anisotropic policy test, which runs in float64) and no precise = 0 case does;
  (c) the Nyquist entry of the odd filter left in (`wavenumber`: k_odd = k_even) -> all 75 cases of test_backward_vs_oracle, all multi-tile
      cases (oracle comparison), all eight Nyquist cases (the leak probe by factors of 37 .. 4300; the analytic part only along y, where
      grad_p becomes 39 .. 620 -- along x the leak of g_u lands in the unused half of the packed pair), both autograd cases and the
      anisotropic policy test fail.
The guard-band tests and the bitwise policy tests pass under all three: they compare the library with itself.
"""
import collections
import functools
import math

import numpy as np
import torch

from oracle import periodic as OP

DT, RHO, LX, LY = 1.0, 1.3, 1.5, 4.0
FFT_LENGTHS = (64, 128, 256, 512, 1024)
GRID_CAP = 512                # spec_grid_cap()
AMP_MAX = 8.0                 # kF32AmpMax
NORTH_STAR = 1e-5
FLOOR = 1e-6
E32_LIMIT = 2e-6
OUTPUTS = ('grad_u', 'grad_v', 'grad_p')
ALL_OUTPUTS = OUTPUTS + ('grad_u_prev', 'grad_v_prev')

Case = collections.namedtuple('Case', 'B nx ny precise A swap')


def lines(n):
    """Lines (columns of an x-pass tile, rows of a y-pass group) per workgroup: SpecLds<N>::LINES."""
    return 8192 // n


def case_id(c):
    return 'B%d-%dx%d-p%d-A%g%s' % (c.B, c.nx, c.ny, c.precise, c.A, '-swap' if c.swap else '')


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.linalg.norm(b.ravel())
    return float(np.linalg.norm((a - b).ravel()) / (d if d > 0 else 1.0))


def lengths(c):
    return (LY, LX) if c.swap else (LX, LY)


def nu_for(A, nx, Lx, ny, Ly):
    n, L = max(((nx, Lx), (ny, Ly)), key=lambda t: t[0] / t[1])
    return A * math.sqrt(3.0) * L / (math.pi * n)


def params(c):
    """(dt, Lx, Ly, rho, nu) of a case."""
    Lx, Ly = lengths(c)
    return DT, Lx, Ly, RHO, nu_for(c.A, c.nx, Lx, c.ny, Ly)


# ------------------------------------------------------------------------------------------------------------------ the cases
ARITH = ((0, 0.1), (0, 4.0), (2, 0.1), (2, 4.0), (2, 20.0))          # (precise, A)
XPASS_SHAPES = [(2, N, 100) for N in FFT_LENGTHS]                   # FFT along x, y dense: every tile width 128 .. 8 has a ragged last column tile
YPASS_SHAPES = [(3, 7, N) for N in FFT_LENGTHS]                     # x dense, 21 rows: a partial last row group at every N
PAIR_SHAPES = [(2, 64, 1024, False), (1, 1024, 64, True), (1, 128, 512, False), (1, 512, 128, True), (1, 256, 256, False)]      # (..., swap)
CASES = ([Case(*s, p, A, False) for s in XPASS_SHAPES + YPASS_SHAPES for p, A in ARITH]
         + [Case(*s[:3], p, A, s[3]) for s in PAIR_SHAPES for p, A in ARITH])
GUARD_CASES = [c for c in CASES if c.A == 4.0 and (c.B, c.nx, c.ny) in ((2, 64, 100), (3, 7, 64), (2, 1024, 100), (3, 7, 1024))]
AUTOGRAD_CASES = [Case(2, 64, 100, 0, 4.0, False), Case(2, 64, 100, 2, 4.0, False)]
POLICY_SHAPES = [(1, 256, 256), (2, 128, 100), (3, 7, 512)]
ANISO_SHAPE, ANISO_L, ANISO_AMP_Y = (1, 64, 1024), 1.5, 12.0         # Lx = Ly: amplification 12 along y, 12 * 64 / 1024 = 0.75 along x
# (case, the pass it is there for, what it reaches)
MULTI = [
    (Case(1100, 64, 64, 0, 4.0, False), 'x', '1100 column tiles of which half the columns are masked; 550 row groups'),
    (Case(140, 1024, 64, 0, 4.0, False), 'x', '1120 column tiles of width 8; 1120 row groups'),
    (Case(280, 256, 100, 0, 4.0, False), 'x', '1120 column tiles, every fourth ragged, mid-pipeline'),
    (Case(600, 7, 1024, 2, 20.0, False), 'y', '525 float64 row groups, the last one full'),
    (Case(601, 7, 1024, 2, 20.0, False), 'y', '526 float64 row groups with a partial last one'),
    (Case(140, 1024, 64, 2, 20.0, False), 'x', "float64 column kernel's grid-stride loop"),
]


# ------------------------------------------------------------------------------------------------------------------ dispatch, restated
def is_fft(n):
    return n in FFT_LENGTHS


def amplification(nu, n, L):
    return abs(nu) * math.pi * n / (math.sqrt(3.0) * abs(L))


def resolved_f32(precise, nu, nx, Lx, ny, Ly):
    """spec_resolve_precise: float32 transforms only if every FFT axis allows them."""
    ok = lambda n, L: (not is_fft(n)) or precise == 0 or (precise == 1 and amplification(nu, n, L) <= AMP_MAX)
    return ok(nx, Lx) and ok(ny, Ly)


def _strided(work):
    wgs = min(work, GRID_CAP)
    return dict(workgroups=wgs, max_per_workgroup=-(-work // wgs))


def dispatch(c):
    """What one call of the case launches: {'f32', 'amp_x', 'amp_y', 'x': {...}, 'y': {...}}."""
    dt, Lx, Ly, rho, nu = params(c)
    f32 = resolved_f32(c.precise, nu, c.nx, Lx, c.ny, Ly)
    if is_fft(c.nx):
        w = lines(c.nx)
        per_grid = -(-c.ny // w)
        x = dict(kernel='xsplit_f32' if f32 else 'xpass_f64', lines=w, tiles_per_grid=per_grid, tiles=c.B * per_grid, ragged=c.ny % w != 0,
                 **_strided(c.B * per_grid))
    else:
        x = dict(kernel='dense')
    if is_fft(c.ny):
        w = lines(c.ny)
        rows = c.B * c.nx
        y = dict(kernel='ypass_f32' if f32 else 'ypass_f64', lines=w, rows=rows, tiles=-(-rows // w), partial_tail=rows % w != 0,
                 **_strided(-(-rows // w)))
    else:
        y = dict(kernel='dense')
    return dict(f32=f32, amp_x=amplification(nu, c.nx, Lx), amp_y=amplification(nu, c.ny, Ly), x=x, y=y)


def paths(c):
    """The kernels of a case, under the names the measured figures are kept by."""
    d = dispatch(c)
    names = {'xsplit_f32': 'float32 x-split', 'xpass_f64': 'float64 x', 'ypass_f32': 'float32 y', 'ypass_f64': 'float64 y', 'dense': 'dense-mixed'}
    return sorted({names[d['x']['kernel']], names[d['y']['kernel']]})


def chunks(c):
    """Consecutive batch pieces [(b0, b1), ...] small enough that no workgroup of either pass gets a second tile; the first boundary is odd."""
    d = dispatch(c)
    most = c.B
    if d['x']['kernel'] != 'dense':
        most = min(most, GRID_CAP // d['x']['tiles_per_grid'])
    if d['y']['kernel'] != 'dense':
        most = min(most, GRID_CAP * d['y']['lines'] // c.nx)
    first = most if most % 2 else most - 1
    edges = [0, first]
    while edges[-1] < c.B:
        edges.append(min(edges[-1] + most, c.B))
    return list(zip(edges[:-1], edges[1:]))


def compared_grids(c):
    """First, one interior, last: under the kernels' last-grid-first tile order they lie in three different iterations of a multi-tile launch."""
    return sorted({0, c.B // 2, c.B - 1})


# ------------------------------------------------------------------------------------------------------------------ inputs
def _noise_filter(nx, ny):
    mx = torch.fft.fftfreq(nx, 1.0 / nx, dtype=torch.float64)[:, None]
    my = torch.fft.rfftfreq(ny, 1.0 / ny, dtype=torch.float64)[None, :]
    return 1.0 / (1.0 + torch.sqrt(mx * mx + my * my))


def make_fields(nx, ny, grids):
    """(u, v, g_u, g_v, g_div), each [len(grids), nx, ny] float32: grid b is the same whatever batch it is asked for in."""
    w = torch.empty(len(grids), 5, nx, ny, dtype=torch.float64)
    for i, b in enumerate(grids):
        g = torch.Generator().manual_seed(1000003 * nx + 7919 * ny + 15485863 * b + 11)
        w[i] = torch.randn(5, nx, ny, generator=g)                # float32 draws: five times as fast as float64 ones, and white all the same
    with _few_threads(w.numel()):
        f = torch.fft.irfft2(torch.fft.rfft2(w) * _noise_filter(nx, ny), s=(nx, ny))
        f = f / f.abs().amax(dim=(2, 3), keepdim=True)
    return tuple(f[:, k].float().contiguous() for k in range(5))


@functools.lru_cache(maxsize=None)
def _fields_cached(nx, ny, grids):
    return make_fields(nx, ny, grids)


def fields(c, grids=None):
    """The case's five fields (cached and shared: leave them unchanged), or those of some of its grids."""
    return _fields_cached(c.nx, c.ny, tuple(range(c.B)) if grids is None else tuple(grids))


# ------------------------------------------------------------------------------------------------------------------ the reference
def oracle_of(f, prm):
    """oracle.periodic.spectral_residual_vjp in float64: {'grad_u', ..., 'grad_v_prev'} as float64 numpy."""
    return dict(zip(ALL_OUTPUTS, OP.spectral_residual_vjp(*[t.double().numpy() for t in f], *prm)))


@functools.lru_cache(maxsize=None)
def _oracle_cached(nx, ny, grids, prm):
    return oracle_of(_fields_cached(nx, ny, grids), prm)


def oracle(c, grids=None):
    return _oracle_cached(c.nx, c.ny, tuple(range(c.B)) if grids is None else tuple(grids), params(c))


def expected_prev(g, dt):
    """grad_u_prev / grad_v_prev, exactly: -(g * float32(1 / dt)) in float32."""
    return -(g * torch.tensor(1.0 / dt, dtype=torch.float32))


MUTATIONS = ('swap_L', 'visc_sign', 'drop_gdiv', 'rho_one', 'drop_pointwise', 'swap_uy_vx', 'drop_flux', 'nyquist_packed')


def mutation_applies(mutation, nx, Lx, ny, Ly):
    if mutation == 'swap_L':
        return Lx != Ly
    if mutation == 'nyquist_packed':
        return is_fft(nx) or is_fft(ny)
    return True


def _wavenumbers(n, L, dtype):
    k = 2 * math.pi * torch.fft.fftfreq(n, d=L / n, dtype=torch.float64)
    k1 = k.clone()
    if n % 2 == 0:
        k1[n // 2] = 0.0
    return k1.to(dtype), k.to(dtype)


def _nyquist_leak(h, axis, n, L):
    """What the partner h of a packed pair adds to the other field's derivative when the Nyquist wavenumber k_N = -(n / 2)(2 pi / L) is kept:
    -k_N H_N (-1)^j, H_N the Nyquist amplitude of h along the axis."""
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).to(h.dtype)
    sign = sign[:, None] if axis == -2 else sign[None, :]
    k_n = -(n / 2) * (2 * math.pi / L)
    return -k_n * (h * sign).mean(dim=axis, keepdim=True) * sign


class _few_threads(object):
    """Small transforms on one thread: torch's CPU FFT loses a factor of ten and more to its thread pool below a million points."""

    def __init__(self, points):
        self.n = 1 if points < (1 << 20) else None

    def __enter__(self):
        self.saved = torch.get_num_threads()
        if self.n:
            torch.set_num_threads(self.n)

    def __exit__(self, *exc):
        torch.set_num_threads(self.saved)
        return False


def vjp(f, prm, dtype=torch.float64, mutation=None):
    with _few_threads(f[0].numel()):
        return _vjp(f, prm, dtype, mutation)


def _vjp(f, prm, dtype, mutation):
    """The oracle's formula (oracle.periodic.residual_vjp with spectral_derivs) in torch, computed in `dtype`: without a mutation and in
    float64 it IS the oracle to rounding (asserted in test_oracle_specbwd.py), so a mutant differs by its mutation alone.  Returns the three
    gradients as float64 numpy."""
    u, v, a, b, d = [t.to(dtype) for t in f]
    dt, Lx, Ly, rho, nu = prm
    if mutation == 'swap_L':
        Lx, Ly = Ly, Lx
    if mutation == 'rho_one':
        rho = 1.0
    if mutation == 'visc_sign':
        nu = -nu
    if mutation == 'drop_gdiv':
        d = torch.zeros_like(d)
    nx, ny = u.shape[-2:]
    nyh = ny // 2 + 1
    kx1, kx = [k[:, None] for k in _wavenumbers(nx, Lx, dtype)]
    ky1, ky = [k[None, :nyh] for k in _wavenumbers(ny, Ly, dtype)]
    back = lambda F: torch.fft.irfft2(F, s=(nx, ny))
    dx = lambda h: back(1j * (kx1 * torch.fft.rfft2(h)))
    dy = lambda h: back(1j * (ky1 * torch.fft.rfft2(h)))
    lap = lambda h: back(-(kx * kx + ky * ky) * torch.fft.rfft2(h))
    ux, uy, vx, vy = dx(u), dy(u), dx(v), dy(v)
    aux, avy, bux, bvy = dx(a * u), dy(a * v), dx(b * u), dy(b * v)
    ax, by, ddx, ddy = dx(a), dy(b), dx(d), dy(d)
    if mutation == 'nyquist_packed':
        if is_fft(nx):                                            # pairs (u, v), (a, b), (a u + d, b u)
            leak = lambda h: _nyquist_leak(h, -2, nx, Lx)
            ux, vx, ax = ux + leak(v), vx - leak(u), ax + leak(b)
            aux, bux = aux + leak(b * u), bux - leak(a * u + d)
        if is_fft(ny):                                            # pairs (u, v), (a, b), (a v, b v + d)
            leak = lambda h: _nyquist_leak(h, -1, ny, Ly)
            uy, vy, by = uy + leak(v), vy - leak(u), by - leak(a)
            avy, bvy = avy + leak(b * v + d), bvy - leak(a * v)
    if mutation == 'swap_uy_vx':
        uy, vx = vx, uy
    if mutation == 'drop_flux':
        aux = avy = bux = bvy = torch.zeros_like(u)
    pointwise = torch.zeros_like(u) if mutation == 'drop_pointwise' else a * ux + b * vx
    grad_u = a / dt + pointwise - aux - avy - nu * lap(a) - ddx
    grad_v = b / dt + a * uy + b * vy - bux - bvy - nu * lap(b) - ddy
    grad_p = -(ax + by) / rho
    return dict(zip(OUTPUTS, [t.double().numpy() for t in (grad_u, grad_v, grad_p)]))


def worst(got, ref):
    return max(rel_l2(got[q], ref[q]) for q in OUTPUTS)


@functools.lru_cache(maxsize=None)
def _e32_cached(nx, ny, grids, prm):
    return worst(vjp(_fields_cached(nx, ny, grids), prm, torch.float32), _oracle_cached(nx, ny, grids, prm))


def e32(c, grids=None):
    """The largest rel-L2, over the three gradients, between the oracle's formula in float32 and the float64 oracle."""
    return _e32_cached(c.nx, c.ny, tuple(range(c.B)) if grids is None else tuple(grids), params(c))


def bound(c, grids=None):
    if c.precise == 0:
        d = dispatch(c)
        assert max(d['amp_x'] if is_fft(c.nx) else 0.0, d['amp_y'] if is_fft(c.ny) else 0.0) <= AMP_MAX, case_id(c)
        return NORTH_STAR
    assert c.precise == 2, case_id(c)
    return min(NORTH_STAR, max(10 * e32(c, grids), FLOOR))


def mutant(mutation, c, grids=None):
    return vjp(fields(c, grids), params(c), torch.float64, mutation)


# ------------------------------------------------------------------------------------------------------------------ single modes
NYQUIST_CASES = [(N, axis, p) for N in (64, 1024) for axis in ('x', 'y') for p in (0, 2)]
NYQUIST_A = 4.0


def nyquist_setup(N, axis):
    """(shape, (dt, Lx, Ly, rho, nu), the Nyquist mode cos(N/2 2 pi s / L) = (-1)^j along `axis` as [1, nx, ny] float32, k_N)."""
    nx, ny = (N, 64) if axis == 'x' else (64, N)
    nu = nu_for(NYQUIST_A, nx, LX, ny, LY)
    j = torch.arange(N)
    mode = torch.where(j % 2 == 0, 1.0, -1.0)
    mode = (mode[:, None] if axis == 'x' else mode[None, :]).expand(nx, ny)[None].float().contiguous()
    k_n = (N // 2) * 2 * math.pi / (LX if axis == 'x' else LY)
    return (1, nx, ny), (DT, LX, LY, RHO, nu), mode, k_n


def leak_probe(N, axis):
    """u a Nyquist mode along `axis`, v a low mode, g_u = 1, g_v = 0.5, g_div = 0: a packed transform that keeps the Nyquist wavenumber would put
    u's mode, times k_N, into v's derivative (seen through g_v v_x, g_v v_y) and g_v u's into the derivative of g_u u."""
    shape, prm, mode, _ = nyquist_setup(N, axis)
    _, nx, ny = shape
    x = torch.arange(nx, dtype=torch.float64)[:, None] / nx
    y = torch.arange(ny, dtype=torch.float64)[None, :] / ny
    low = (torch.sin(2 * math.pi * (3 * x + 0.1)) * torch.cos(2 * math.pi * (2 * y + 0.3)))[None].float().contiguous()
    one = torch.ones(shape)
    return prm, (mode, low, one, 0.5 * one, torch.zeros(shape))
