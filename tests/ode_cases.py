"""Cases of the fused ODEFunc integrator (tests/test_gpu_ode_mlp.py runs them on the GPU; tests/test_oracle_neural.py runs every condition
on the reference alone, without one).

Dispatch (csrc/ode_mlp_kernels.hip, nns/neural_spectral/anode.py), restated:
  forward   nns_ode_mlp_fwd_f32: mb <= NNS_ODE_ROW_MAX (environment, read once per process, default 4096) -> ode_mlp_fwd_row_kernel, one batch
            row per workgroup, weights in registers; otherwise ode_mlp_fwd_kernel, 16-row MFMA tiles.  NNS_ODE_ROW_MAX=0 forces the tile kernel.
  backward  _OdeMlpFn.backward: Nt > 1 and mb * Nt * K <= anode._parallel_rows (2 * cu_count * 16 unless set) -> TIME-PARALLEL: the step
            Jacobians by nns_ode_mlp_bwd_steps_f32 without parameter gradients, nns_ode_adjoint_chain_f32, then nns_ode_mlp_bwd_steps_f32 with
            them; otherwise SEQUENTIAL: one nns_ode_mlp_bwd_f32 launch.  Both are ode_mlp_bwd_kernel: 16-row tiles, parameter gradients by
            atomics (one per address and workgroup).
The GPU tests call ops.ode_mlp_fwd / ode_mlp_bwd / ode_mlp_bwd_steps directly, force the tile forward in a child process and set
anode._parallel_rows, so the card's CU count never chooses the kernel.

Inputs of case (K, mb, Nt), from one torch.Generator seeded from the case: weights N(0, 1 / fan_in), b0 and b1 N(0, 0.3^2), b2 N(0, 0.1^2),
z0 N(0, 1), upstream weight w [Nt, mb, K] N(0, 1); the loss is (out * w).sum().  Conditions asserted on the reference alone
(test_oracle_neural.py): at the first stage the share of live ReLU units and the share of negative ELU pre-activations lie in [0.3, 0.7], and
e32 -- the largest rel-L2, over the trajectory and the seven gradients, between the oracle in float32 and in float64 -- is <= 1e-6 (weights
three times as large flip ReLU kinks between the two: 2e-5).

Bound: a GPU result is within max(10 * e32(case, scheme), 2e-6) rel-L2 of the float64 oracle.  The kernels differ from the float32 oracle in
the order of their sums and by elu1 (documented at 5e-7 relative per evaluation); the factor 10 is a margin, not a measurement.  The same rule
gives the bound of the independent single steps (`step_bound`).  Three deliberately wrong float64 oracles miss the bound by >= 100 x
(`mutant`): RK4 weights 1/6 and 1/3 exchanged, ELU derivative 1 for z < 0, row mb - 1 left out of the parameter gradients.

Measured on an MI355X: the worst rel-L2 against the float64 oracle over all cases, schemes and quantities of a path, and the path's smallest
margin bound / error (two runs; with three or more row tiles the order of the atomics moves the last digit):
  path                                 worst error                             smallest margin
  row forward                          3.2e-7  traj  K30 mb5 Nt60 RK4          14 x   (the same)
  tile forward                         3.3e-7  traj  K30 mb5 Nt60 RK4          14 x   (the same)
  sequential backward                  5.8e-7  gW2   K30 mb5 Nt60 RK4          5.5 x  gb2  K2 mb16 Nt3 Euler   (3.6e-7 of 2e-6)
  independent steps (dt = 0.013)       3.1e-7  gb2   K1 rows250 RK4            10 x   gb0  K1 rows17 RK2       (2.1e-7 of 2.2e-6)
  time-parallel backward               5.2e-7  gb2   K2 mb16 Nt3 RK4           3.9 x  (the same, of 2e-6)
Nothing exceeded its bound; nothing in the kernels was changed.  Exactly 0 came out where it has to: gb2 of one Euler step (dt * grad_out summed
over one row) at K1 mb1 Nt1 and K16 mb1 Nt1.

elu1 read out exactly (`elu_readout`: K = 32, mb = 1, Euler, Nt = 1, everything zero but b1 and a one-hot W2, so out[j] is bit for bit
elu1(b1[32 q + j])) on `elu_points()`, 2048 values of z in [-110, 2]: z > 0 comes back bitwise, z <= -18 gives exactly -1, and against float64
expm1 of the float32 input the relative error is at most 1.25e-7, at z = -0.359560013 on the exp2 branch (8.8e-8 at z = -6.03e-8 on the
polynomial branch) -- the same figures from the row and from the tile kernel, a quarter of the 5e-7 the kernel's comment claims and an eighth
of the 1e-6 asserted.  The derivative h + 1, read out through gb1 of ops.ode_mlp_bwd, is within 5.2e-8 absolute of exp(min(z, 0)) (at
z = -0.34708; 6e-7 asserted).  Subnormal z come back as they went in: nothing on either path flushes them.

What the bound and the read-outs reject, run once against deliberately wrong builds of the kernels (each change in bounds, none kept): ELU
derivative taken as 1 in ode_mlp_bwd_kernel -> every backward test of every path and the derivative read-out fail; the last RK4 weight of
the tile forward 1/3 for 1/6 -> the ten RK4 tile-forward cases fail and nothing else; elu1's polynomial used down to z = -1 (2.7e-6 relative
at its end) -> both elu1 read-outs fail while all sixty trajectories stay inside their bounds, which is what the read-out is for.
"""
import functools
import math

import numpy as np
import torch

from oracle import neural as ON

H = 128                       # hidden width of ODEFunc
TB = 16                       # batch rows per workgroup of the tile kernels
METHODS = ('Euler', 'RK2', 'RK4')
GRADS = ('gz0', 'gW0', 'gb0', 'gW1', 'gb1', 'gW2', 'gb2')
QUANTITIES = ('traj',) + GRADS

# (K, mb, Nt, the edge it is there for)
CASES = [
    (1, 1, 1, 'one column, one row, one step: backward reads z0 only'),
    (1, 17, 2, 'K=1, second tile holds a single real row'),
    (2, 16, 3, 'exactly one full tile'),
    (15, 15, 4, 'one short of the 16-column MFMA tile and of the 16-row tile'),
    (16, 1, 1, 'second layer-3 column tile entirely padding'),
    (17, 33, 5, 'one column into the second column tile; three row tiles, the last with 1 row'),
    (31, 17, 3, 'one padded column'),
    (32, 16, 2, 'no padding anywhere'),
    (32, 49, 4, 'four row tiles: atomics from four workgroups'),
    (30, 5, 60, "the workload's K over a longer horizon"),
]
SHAPES = [c[:3] for c in CASES]
CASE_METHODS = [c[:3] + (m,) for c in CASES for m in METHODS]
FLOOR = 2e-6
E32_LIMIT = 1e-6


def case_id(K, mb, Nt, method=None):
    return 'K%d-mb%d-Nt%d' % (K, mb, Nt) + ('-' + method if method else '')


CASE_METHOD_IDS = [case_id(*c) for c in CASE_METHODS]


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.linalg.norm(b.ravel())
    return float(np.linalg.norm((a - b).ravel()) / (d if d > 0 else 1.0))


# ------------------------------------------------------------------------------------------------------------------ inputs
def _mlp(g, K):
    return (torch.randn(H, K, generator=g) / math.sqrt(K), 0.3 * torch.randn(H, generator=g),
            torch.randn(H, H, generator=g) / math.sqrt(H), 0.3 * torch.randn(H, generator=g),
            torch.randn(K, H, generator=g) / math.sqrt(H), 0.1 * torch.randn(K, generator=g))


@functools.lru_cache(maxsize=None)
def inputs(K, mb, Nt):
    """(mlp = (W0, b0, W1, b1, W2, b2), z0 [mb, K], w [Nt, mb, K]): float32, CPU.  Shared: leave them unchanged.
    (The seed's last term: without it the draw of case (1, 17, 2) has a gb2 -- with K = 1 a single number, the sum of 17 x 2 x 4 adjoint terms
    -- that cancels to 0.03 of terms of order 1, and e32 of that one number is 2e-5.  Five other offsets gave 3.9e-7 .. 6.1e-7 at worst.)"""
    g = torch.Generator().manual_seed(1000003 * K + 7919 * mb + Nt + 104729)
    mlp = _mlp(g, K)
    return mlp, torch.randn(mb, K, generator=g), torch.randn(Nt, mb, K, generator=g)


def first_stage_shares(K, mb, Nt):
    """(share of live ReLU units, share of negative ELU pre-activations) of the first MLP evaluation, float64."""
    (W0, b0, W1, b1, _, _), z0, _ = inputs(K, mb, Nt)
    z1 = z0.double() @ W0.double().t() + b0.double()
    z2 = torch.relu(z1) @ W1.double().t() + b1.double()
    return float((z1 > 0).double().mean()), float((z2 < 0).double().mean())


# ------------------------------------------------------------------------------------------------------------------ the reference
def _leaves(ts, dtype):
    return tuple(t.to(dtype).clone().requires_grad_(True) for t in ts)


def _collect(traj, z, mlp):
    return dict(zip(QUANTITIES, [t.detach().double().numpy() for t in (traj, z.grad) + tuple(p.grad for p in mlp)]))


@functools.lru_cache(maxsize=None)
def oracle(K, mb, Nt, method, dtype=torch.float64):
    """oracle.neural.integrate and autograd of (out * w).sum(), computed in `dtype`: {'traj', 'gz0', 'gW0', ..., 'gb2'} as float64 numpy."""
    mlp32, z0, w = inputs(K, mb, Nt)
    mlp, (z,) = _leaves(mlp32, dtype), _leaves((z0,), dtype)
    traj = ON.integrate(mlp, z, Nt, method)
    (traj * w.to(dtype)).sum().backward()
    return _collect(traj, z, mlp)


def _worst(got, ref, names=QUANTITIES):
    return max(rel_l2(got[q], ref[q]) for q in names)


@functools.lru_cache(maxsize=None)
def e32(K, mb, Nt, method):
    return _worst(oracle(K, mb, Nt, method, torch.float32), oracle(K, mb, Nt, method))


def bound(K, mb, Nt, method):
    return max(10 * e32(K, mb, Nt, method), FLOOR)


# ------------------------------------------------------------------------------------------------------------------ wrong oracles
MUTATIONS = ('rk4_weights', 'elu_grad', 'drop_row')


class _EluGradOne(torch.autograd.Function):
    """ELU whose derivative is taken as 1 for z < 0."""

    @staticmethod
    def forward(ctx, z):
        return torch.nn.functional.elu(z)

    @staticmethod
    def backward(ctx, g):
        return g


def _odefunc_elu_grad_one(mlp, y):
    W0, b0, W1, b1, W2, b2 = mlp
    return _EluGradOne.apply(torch.relu(y @ W0.t() + b0) @ W1.t() + b1) @ W2.t() + b2


def _integrate_with(f, y, Nt, method, c_outer=1.0 / 6.0, c_inner=1.0 / 3.0):
    dt = 1. / float(Nt)
    out = []
    for _ in range(Nt):
        if method == 'Euler':
            y = y + dt * f(y)
        elif method == 'RK2':
            y = y + dt * f(y + 0.5 * (dt * f(y)))
        else:
            k1 = dt * f(y)
            k2 = dt * f(y + 0.5 * k1)
            k3 = dt * f(y + 0.5 * k2)
            k4 = dt * f(y + k3)
            y = y + c_outer * k1 + c_inner * k2 + c_inner * k3 + c_outer * k4
        out.append(y)
    return torch.stack(out)


def mutation_acts(mutation, K, mb, Nt, method):
    return {'rk4_weights': method == 'RK4', 'elu_grad': True, 'drop_row': mb > 1}[mutation]


def mutation_quantities(mutation, Nt, method):
    """The quantities a mutation has to move by 100 x the bound.  With one Euler step gW2 and gb2 never meet the ELU derivative.  RK4 with its
    weights exchanged is still a consistent second-order scheme (the weights sum to 1, sum b_i c_i = 1/2): at dt = 1/60 it moves the
    trajectory by 3.7e-6 only, 0.8 x the bound, and it is the gradients (120 x .. 680 x) that reject it there."""
    if mutation == 'rk4_weights':
        return QUANTITIES if Nt <= 5 else GRADS
    if mutation == 'elu_grad':
        return GRADS if (Nt > 1 or method != 'Euler') else GRADS[:5]
    return GRADS[1:]


@functools.lru_cache(maxsize=None)
def mutant(mutation, K, mb, Nt, method):
    """A deliberately wrong float64 oracle, same form as `oracle`.  _integrate_with without a mutation IS the oracle (asserted in
    test_oracle_neural.py), so what a mutant differs by is its mutation alone."""
    mlp32, z0, w = inputs(K, mb, Nt)
    mlp, (z,) = _leaves(mlp32, torch.float64), _leaves((z0,), torch.float64)
    f = lambda y: ON.odefunc(mlp, y)
    if mutation is None:
        traj = _integrate_with(f, z, Nt, method)
    elif mutation == 'rk4_weights':
        traj = _integrate_with(f, z, Nt, method, c_outer=1.0 / 3.0, c_inner=1.0 / 6.0)
    elif mutation == 'elu_grad':
        traj = _integrate_with(lambda y: _odefunc_elu_grad_one(mlp, y), z, Nt, method)
    elif mutation == 'drop_row':
        cut = tuple(p.detach() for p in mlp)
        traj = torch.cat([_integrate_with(f, z[:-1], Nt, method), _integrate_with(lambda y: ON.odefunc(cut, y), z[-1:], Nt, method)], dim=1)
    else:
        raise ValueError(mutation)
    (traj * w.double()).sum().backward()
    return _collect(traj, z, mlp)


# ------------------------------------------------------------------------------------------------------------------ independent single steps
STEP_ROWS = (1, 16, 17, 250)
STEP_KS = (1, 17, 32)
STEP_DT = 0.013               # not 1 / Nt of anything
STEP_CASES = [(K, rows, m) for K in STEP_KS for rows in STEP_ROWS for m in METHODS]
STEP_IDS = ['K%d-rows%d-%s' % c for c in STEP_CASES]
STEP_GRADS = ('gy',) + GRADS[1:]


@functools.lru_cache(maxsize=None)
def step_inputs(K, rows):
    """(mlp, y [rows, K], g [rows, K]): float32, CPU."""
    g = torch.Generator().manual_seed(2000003 * K + 104729 * rows + 5)
    mlp = _mlp(g, K)
    return mlp, torch.randn(rows, K, generator=g), torch.randn(rows, K, generator=g)


@functools.lru_cache(maxsize=None)
def step_oracle(K, rows, method, dtype=torch.float64):
    """grad_y[r] = (dy'[r] / dy[r])^T g[r] and the parameter gradients summed over the rows, of y' = oracle.neural.step(mlp, y, STEP_DT)."""
    mlp32, y0, g = step_inputs(K, rows)
    mlp, (y,) = _leaves(mlp32, dtype), _leaves((y0,), dtype)
    (ON.step(mlp, y, STEP_DT, method) * g.to(dtype)).sum().backward()
    return dict(zip(STEP_GRADS, [t.grad.detach().double().numpy() for t in (y,) + mlp]))


@functools.lru_cache(maxsize=None)
def step_e32(K, rows, method):
    return _worst(step_oracle(K, rows, method, torch.float32), step_oracle(K, rows, method), STEP_GRADS)


def step_bound(K, rows, method):
    return max(10 * step_e32(K, rows, method), FLOOR)


# ------------------------------------------------------------------------------------------------------------------ elu1, read out exactly
ELU_K = 32
ELU_SPLIT = -0.35             # elu1: exp2 at and below, the polynomial above
ELU_EXACT_MINUS_ONE = -18.0   # exp(z) < 2^-25 from z = -17.33 on: 1 - exp(z) rounds to 1 in float32
ELU_REL = 1e-6                # twice the 5e-7 the kernel's comment claims
ELU_GRAD_ABS = 6e-7           # |h| <= 1 times that claim, plus one float32 rounding of h + 1


def _neighbours(v, n):
    """The n float32 values on both sides of v, and v."""
    out, lo, hi = [np.float32(v)], np.float32(v), np.float32(v)
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


@functools.lru_cache(maxsize=None)
def elu_points():
    """[16, 128] float32 in [-110, 2]: 0 and ELU_SPLIT with their float32 neighbours, the subnormal / normal edge, powers of ten, dense ramps
    around 0 and ELU_SPLIT, a logarithmic ramp down to the underflow region, the region itself, and a uniform rest."""
    v = [np.float32(-0.0)] + _neighbours(0.0, 8) + _neighbours(ELU_SPLIT, 16)
    tiny = float(np.finfo(np.float32).tiny)
    v += _neighbours(tiny, 2) + _neighbours(-tiny, 2)
    v += [s * 10.0 ** e for e in range(-38, 0) for s in (1, -1)]
    v += [-17.0, -17.25, -17.32, -17.33, -17.34, -17.5, -18.0, -19.0, -20.0, -30.0, -50.0, -80.0, -87.0, -87.5, -88.0, -89.0, -100.0, -103.0,
          -104.0, -105.0, -110.0, 1.0, 2.0, -1.0, -2.0]
    v += list(np.linspace(ELU_SPLIT - 0.01, ELU_SPLIT + 0.01, 501)) + list(np.linspace(-0.005, 0.005, 401))
    v += list(-np.logspace(-8, math.log10(110.0), 400)) + list(np.logspace(-8, math.log10(2.0), 100))
    v += list(np.linspace(-2.0, 2.0, 257))
    v = np.array(v, dtype=np.float32)
    n = 16 * H
    assert len(v) < n
    v = np.concatenate([v, np.linspace(-110.0, 2.0, n - len(v)).astype(np.float32)])
    v = v[np.random.RandomState(5).permutation(n)]                       # every kind of value in every quarter of the hidden units
    assert v.min() == -110.0 and v.max() == 2.0 and len(np.unique(v)) > 2000
    return torch.from_numpy(v.reshape(16, H).copy())


def elu_expected(z):
    """float64 expm1 of the float32 input for z <= 0, z itself above."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


def elu_setup(b1, q, device):
    """The arguments (z0, W0, b0, W1, b1, W2, b2) that route elu1(b1[32 q + j]) to output j."""
    z = lambda *s: torch.zeros(*s, device=device)
    W2 = z(ELU_K, H)
    W2[torch.arange(ELU_K), 32 * q + torch.arange(ELU_K)] = 1.
    return z(1, ELU_K), z(H, ELU_K), z(H), z(H, H), b1.to(device).contiguous(), W2, z(ELU_K)


def elu_readout(ops, points):
    """elu1 of every value of points [n, 128] as the forward kernel of this process computes it: [n, 128] float32, CPU."""
    out = torch.empty_like(points)
    for i, b1 in enumerate(points):
        for q in range(H // 32):
            out[i, 32 * q:32 * q + 32] = ops.ode_mlp_fwd(*elu_setup(b1, q, 'cuda'), 1, 'Euler').cpu()[0, 0]
    return out


def elu_errors(z, got):
    """(relative error against float64 expm1 where z < 0, the mask of those points) after asserting what has to hold exactly."""
    z, got = np.asarray(z, dtype=np.float32).ravel(), np.asarray(got, dtype=np.float32).ravel()
    pos, zero, neg = z > 0, z == 0, z < 0
    assert np.array_equal(got[pos].view(np.int32), z[pos].view(np.int32)), 'z > 0 must come back bitwise'
    assert np.all(got[zero] == 0)
    deep = z <= ELU_EXACT_MINUS_ONE
    assert deep.sum() > 100 and np.all(got[deep] == -1.0), z[deep][got[deep] != -1.0][:8]
    want = elu_expected(z)
    return np.abs(got[neg].astype(np.float64) - want[neg]) / np.abs(want[neg]), neg


# ------------------------------------------------------------------------------------------------------------------ the tile-forward child
def tile_child(path):
    """Runs in a process of its own with NNS_ODE_ROW_MAX=0: every case and scheme and the elu1 read-out through ode_mlp_fwd_kernel, one .npz."""
    import os
    assert os.environ.get('NNS_ODE_ROW_MAX') == '0'
    from nns import ops
    out = {}
    for K, mb, Nt, method in CASE_METHODS:
        mlp, z0, _ = inputs(K, mb, Nt)
        out[case_id(K, mb, Nt, method)] = ops.ode_mlp_fwd(z0.cuda(), *[p.cuda() for p in mlp], Nt, method).cpu().numpy()
    out['elu'] = elu_readout(ops, elu_points()).numpy()
    np.savez(path, **out)
