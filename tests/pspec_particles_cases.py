"""Cases of the periodic solver's Lagrangian tracers (tests/test_gpu_pspec_particles.py runs them on the GPU against
tests/pspec_particles_oracle.py; tests/test_oracle_pspec_particles.py checks the restatement on the CPU and shows that the GPU bounds would
catch each deliberately wrong variant on these very inputs).

Shapes: 64x64 on the 2 pi box, 64x128 with Lx != Ly (hx != hy), and 1024x64 for one call at the longest axis.  B = 3 grids with different flows
and different mean flows; P = 257 particles per grid (one past a workgroup of 256), and P = 1.  Positions: uniform over +-3 boxes, with the
fixed edge cases of edges() in the first slots of every grid.  Flows: pspec_oracle.random_ic with |m| <= 8 plus a mean flow per grid, dt at
CFL 0.5; the four solvers of KINDS."""
import functools

import numpy as np

import pspec_linear_oracle as LO
import pspec_oracle as O
import pspec_particles_oracle as PO

RHO, NU, SEED = 1.0, 2e-3, 4100
B, P = 3, 257
SQUARE = (64, 64, 2 * np.pi, 2 * np.pi)
OBLONG = (64, 128, 2 * np.pi, 5.0)
WIDE = (1024, 64, 2 * np.pi, 2 * np.pi)
SHAPES = (SQUARE, OBLONG)
MEANS = ((0.3, -0.2), (-0.15, 0.25), (0.0, 0.1))              # the mean flow of every grid
ORDERS = (4, 6)
KINDS = ('plain', 'forced', 'linear', 'buoyant')
SCHEMES = (('rk4', 8), ('heun', 3))
FIELDS = ('u', 'v', 'w', 'theta')

# The GPU's float32 results against the float64 restatement, measured on the MI355X (profiles/pspec_particles_run.json holds the same figures):
#   coefficients and samples: max |gpu - ref| / max |ref| per field, the worst over the shapes, both orders and u, v, w, theta;
#   advect: max |pos - ref| / max |ref - pos0| (the error of the displacement), the worst over KINDS x SCHEMES and both orders.
# Each bound is 4x the worst seen: the allowance for a different FMA order on another build.
MEASURED = {'coef': 1.17e-6,       # w at 64x128, order 6 (u, v, theta: <= 2.8e-7)
            'sample': 3.75e-7,     # w at 64x128, order 6 (u, v, theta: <= 2.2e-7; 1024x64: 1.6e-7)
            'advect': 1.72e-7}     # plain, rk4, 8 steps, order 4 (every run: 1.25e-7 ... 1.72e-7)
COEF_BOUND = 4.6e-6
SAMPLE_BOUND = 1.5e-6
ADVECT_BOUND = 6.8e-7


def shape_id(s):
    return '%dx%d' % s[:2]


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def displacement_error(pos, ref, pos0):
    return float(np.abs(pos - ref).max() / np.abs(ref - pos0).max())


def edges(shape):
    """The fixed positions [E, 2]: a grid node exactly; x = 0; -1e-18 (floor -1, the offset rounds to 1); L (1 - 2^-53); the first and the
    last cell of each axis; 1e6 L."""
    nx, ny, Lx, Ly = shape
    hx, hy = Lx / nx, Ly / ny
    one = 1.0 - 2.0 ** -53
    return np.array([(5 * hx, 7 * hy), (0.0, 0.3 * Ly), (0.3 * Lx, 0.0), (-1e-18, -1e-18), (Lx * one, Ly * one), (0.5 * hx, 0.25 * hy),
                     ((nx - 0.5) * hx, (ny - 0.25) * hy), (0.5 * hx, (ny - 0.25) * hy), (1e6 * Lx + 0.37 * hx, 1e6 * Ly + 0.61 * hy),
                     (-1e6 * Lx + 0.37 * hx, 2.5 * hy)])


@functools.lru_cache(maxsize=None)
def positions(shape, npart=P):
    """float64 [B, npart, 2]: uniform over +-3 boxes, the first slots of every grid the edge cases (as many as fit).  Shared: do not modify."""
    nx, ny, Lx, Ly = shape
    rng = np.random.default_rng(SEED + nx + 3 * ny)
    pos = rng.uniform(-3.0, 3.0, (B, npart, 2)) * np.array([Lx, Ly])
    e = edges(shape)[:npart]
    pos[:, :len(e)] = e
    return pos


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """dict of the float32 fields u0, v0, theta0 [B, nx, ny] and dt.  Shared: do not modify."""
    nx, ny, Lx, Ly = shape
    u, v = O.random_ic(B, nx, ny, 8, SEED + nx + ny, Lx, Ly, 1.0)
    m = np.array(MEANS)
    u, v = u + m[:, 0, None, None], v + m[:, 1, None, None]
    theta = O.random_ic(B, nx, ny, 8, SEED + nx + ny + 1, Lx, Ly, 1.0)[0] + 0.5
    return dict(u0=u.astype(np.float32), v0=v.astype(np.float32), theta0=theta.astype(np.float32), dt=O.cfl_dt(nx, ny, Lx, Ly, 1.5))


def params(kind):
    """The arguments a kind adds to the plain solver, under the restatement's names."""
    return {'plain': {}, 'forced': dict(drag=0.1), 'linear': dict(beta=2.0, hyper=(1e-6, 2)),
            'buoyant': dict(kappa=1e-3, grad=(0.0, 1.0), buoy=(0.0, 1.0))}[kind]


def scheme(kind, shape):
    nx, ny, Lx, Ly = shape
    S = LO.LinearScheme(nx, ny, inputs(shape)['dt'], RHO, NU, Lx, Ly, **params(kind))
    if kind == 'forced':
        S.kolmogorov_forcing(4, 1.0)
    return S


def solver(kind, shape, stochastic=False):
    from nns.periodic import PeriodicSolver
    nx, ny, Lx, Ly = shape
    p = dict(params(kind))
    names = dict(grad='scalar_gradient', buoy='buoyancy', hyper='hyperviscosity')
    s = PeriodicSolver(nx, ny, inputs(shape)['dt'], RHO, NU, Lx, Ly, **{names.get(k, k): v for k, v in p.items()})
    if kind == 'forced':
        s.kolmogorov_forcing(4, 1.0)
    if stochastic:
        s.ring_forcing(0.05, 3.0, 5.0, seed=7)
    return s


def start(kind, shape):
    """(scheme, w, mean, t) of the float64 restatement for the float32 inputs (t None without a scalar)."""
    d, S = inputs(shape), scheme(kind, shape)
    w, mean = S.init(d['u0'], d['v0'])
    return S, w, mean, (S.init_scalar(d['theta0']) if kind == 'buoyant' else None)


@functools.lru_cache(maxsize=None)
def oracle_read(shape, order, wrong=None):
    """(coefficients, samples): dicts by field name of the float64 coefficient images [B, nx, ny] and of the values [B, P] at positions(shape),
    of the buoyant state (it carries all four fields).  Shared: do not modify."""
    S, w, mean, t = start('buoyant', shape)
    T = PO.Tracers(S, order, wrong=wrong)
    pos = positions(shape)
    coef = dict(zip(FIELDS, T.coefficients(w, mean, t, FIELDS)))
    vals = T.sample(w, mean, pos, t, FIELDS)
    return coef, {f: vals[..., k] for k, f in enumerate(FIELDS)}


@functools.lru_cache(maxsize=None)
def oracle_advect(kind, shape, scheme_name, nsteps, order, wrong=None):
    """float64 positions [B, P, 2] after nsteps steps from positions(shape).  Shared: do not modify."""
    S, w, mean, t = start(kind, shape)
    return PO.Tracers(S, order, wrong=wrong).advect(w, mean, positions(shape), nsteps, scheme_name, t)[2]
