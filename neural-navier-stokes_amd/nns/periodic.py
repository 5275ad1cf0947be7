"""Periodic-box incompressible Navier-Stokes residual engine (the north-star hot path).

    r_u   = (u - u_prev)/dt + u u_x + v u_y + p_x/rho - nu lap u
    r_v   = (v - v_prev)/dt + u v_x + v v_y + p_y/rho - nu lap v
    r_div = u_x + v_y

on batches of [B, nx, ny] float32 fields resident in HBM, with two derivative back-ends:
  * 'fd5' / 'fd9'  -- 2nd-order central differences, 5- or 9-point Laplacian (csrc/residual_kernels.hip)
  * 'spectral'     -- Fourier derivatives via LDS-resident FFTs (csrc/spectral_kernels.hip)
The reference has no such operator (motivation
src/neural_spectral/derivations/derivation.tex:25-59); oracle/periodic.py defines it and the
tests pin both back-ends to it (1e-5 rel-L2 in float32).  Axis 0 = x, axis 1 = y.

``precise`` (spectral back-end; include/nns.h): False / 0 = all-float32 transforms of forward-differenced lines, True / 1 = the
library picks that mode while its viscous amplification nu pi N / (sqrt(3) L) stays <= 8 and float64 forward transforms
otherwise, 2 = float64 forward transforms always.

``PeriodicSolver`` produces the trajectories such a residual measures: a pseudo-spectral solver of the same equations on the same box
(csrc/pspec_kernels.hip; scheme and measurements in DESIGN.md).  Its class note is the user documentation; every feature is restated in
float64 by an oracle under tests/:
  * the unforced step                                            pspec_oracle.py
  * steady body force and linear drag                            pspec_forced_oracle.py
  * passive scalar; with ``buoyancy`` it acts on the flow        pspec_scalar_oracle.py, pspec_buoyant_oracle.py
  * ``spectrum`` / ``transfer`` by wavenumber shell              pspec_spectrum_oracle.py
  * white-in-time stochastic forcing made inside the step        pspec_stochastic_oracle.py
  * hyperviscosity, hypofriction, beta in the Lawson factor      pspec_linear_oracle.py
  * reverse mode, ``advance*`` (flow; scalar and buoyancy)       pspec_adjoint_oracle.py, pspec_scalar_adjoint_oracle.py
  * reverse mode on every solver, ``evolve`` / ``evolve_velocity``   pspec_linear_adjoint_oracle.py
  * their ``operator``: gradients in nu, drag, nu_h, mu, beta, lambda(k)   pspec_operator_grad_oracle.py
  * forward mode, ``step_tangent`` / ``evolve_tangent`` / ``lyapunov_exponent``   pspec_tangent_oracle.py
  * K tangents on one base, ``step_tangents`` / ``lyapunov_spectrum``              pspec_lyapunov_oracle.py
  * forward mode with a scalar, ``step_tangent_scalar`` / ``evolve_tangent_scalar``  pspec_scalar_tangent_oracle.py
  * Lagrangian tracers, ``init_particles`` / ``sample`` / ``advect``                 pspec_particles_oracle.py
  * their reverse mode, ``observe`` / ``spread`` / ``sample_gradient``               pspec_particles_adjoint_oracle.py
Which C entry a step, an adjoint or a tangent step takes is decided in one place each: ops.spec_ns_advance_, ops.spec_ns_adjoint_ and
PeriodicSolver._launch_tangent.
"""
import collections
import math
import numbers

import numpy as np
import torch

from . import ops
from ._util import default_device


class ResidualEngine(object):
    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * math.pi, Ly=2 * math.pi, backend='spectral', precise=True):
        if backend not in ('fd5', 'fd9', 'spectral'):
            raise ValueError("backend must be 'fd5', 'fd9' or 'spectral'")
        self.nx, self.ny, self.dt, self.rho, self.nu = nx, ny, dt, rho, nu
        self.Lx, self.Ly = Lx, Ly
        self.dx, self.dy = Lx / nx, Ly / ny
        self.backend, self.precise = backend, precise

    def fd(self, u, v, p, u_prev, v_prev, stencil=5, out=None):
        return ops.fd_residual(u, v, p, u_prev, v_prev, self.dt, self.dx, self.dy, self.rho, self.nu, stencil, out)

    def spectral(self, u, v, p, u_prev, v_prev, out=None):
        return ops.spec_residual(u, v, p, u_prev, v_prev, self.dt, self.Lx, self.Ly, self.rho, self.nu, self.precise, out)

    def __call__(self, u, v, p, u_prev, v_prev, out=None):
        if self.backend == 'spectral':
            return self.spectral(u, v, p, u_prev, v_prev, out)
        return self.fd(u, v, p, u_prev, v_prev, 5 if self.backend == 'fd5' else 9, out)

    def differentiable(self, u, v, p, u_prev, v_prev):
        """The residual as an autograd node (inputs may require grad): forward and backward are both HIP kernels
        (the backward applies the adjoint operators, see oracle/periodic.py: residual_vjp)."""
        if self.backend == 'spectral':
            return ops.SpecResidualFn.apply(u, v, p, u_prev, v_prev, self.dt, self.Lx, self.Ly, self.rho, self.nu, self.precise)
        return ops.FdResidualFn.apply(u, v, p, u_prev, v_prev, self.dt, self.dx, self.dy, self.rho, self.nu, 5 if self.backend == 'fd5' else 9)

    def residual_spec(self):
        """(kind, constants) of this engine's residual as ops.PinnHeadFn takes it."""
        if self.backend == 'spectral':
            return 'spectral', (self.dt, self.Lx, self.Ly, self.rho, self.nu, self.precise)
        return 'fd', (self.dt, self.dx, self.dy, self.rho, self.nu, 5 if self.backend == 'fd5' else 9)

    def physics_loss(self, u, v, p, u_prev, v_prev, w_div=1.0):
        """Mean-square momentum + divergence residual: the physics-informed loss term of SURVEY.md section 8 (f) rank 2
        (hypothesis: src/neural_spectral/derivations/derivation.tex:25-34)."""
        r_u, r_v, r_d = self.differentiable(u, v, p, u_prev, v_prev)
        return (r_u * r_u).mean() + (r_v * r_v).mean() + w_div * (r_d * r_d).mean()

    def both(self, u, v, p, u_prev, v_prev, out_fd=None, out_spec=None, stencil=5, fused=True):
        """The 'stencil + spectral residual' of BASELINE.json: both back-ends on the same inputs.  With the 5-point stencil
        and float32 fields this is nns_residual_both_f32: the spectral column pass and ONE row pass that also
        evaluates the stencil (the inputs cross HBM once less); otherwise, or with fused=False, the two back-ends are
        launched separately.  Same results either way, to rounding."""
        if fused and stencil == 5 and u.dtype == torch.float32:
            return ops.residual_both(u, v, p, u_prev, v_prev, self.dt, self.Lx, self.Ly, self.rho, self.nu, self.precise,
                                     out_fd=out_fd, out_spec=out_spec)
        return (self.fd(u, v, p, u_prev, v_prev, stencil, out_fd), self.spectral(u, v, p, u_prev, v_prev, out_spec))


def _int(name, n):
    if isinstance(n, bool) or not isinstance(n, numbers.Integral):
        raise TypeError("%s must be an int, got %r" % (name, n))
    return int(n)


def _real(name, x, bound=None, kind='be a real number'):
    """x as a finite float; bound '> 0' or '>= 0' also restricts its sign."""
    if isinstance(x, bool) or not isinstance(x, numbers.Real):
        raise TypeError("%s must %s, got %r" % (name, kind, x))
    if bound is None:
        if not math.isfinite(x):
            raise ValueError("%s = %r must be finite" % (name, x))
        return float(x)
    x = float(x)
    if not math.isfinite(x) or (x <= 0 if bound == '> 0' else x < 0):
        raise ValueError("%s = %r must be finite and %s" % (name, x, bound))
    return x


def _pair(name, x, parts):
    """The two finite reals of ``scalar_gradient`` / ``buoyancy``."""
    try:
        a, b = x
    except (TypeError, ValueError):
        raise TypeError("%s must be two real numbers %s, got %r" % (name, parts, x))
    return tuple(_real(name, c, kind='hold real numbers') for c in (a, b))


def _pow2_axis(name, n):
    n = _int(name, n)
    if not (64 <= n <= 1024 and n & (n - 1) == 0):
        raise ValueError("%s = %d: each axis must be a power of two in [64, 1024]" % (name, n))
    return n


def _count(name, n, minimum):
    n = _int(name, n)
    if n < minimum:
        raise ValueError("%s = %d must be >= %d" % (name, n, minimum))
    return n


def _seed(seed):
    seed = _int('seed', seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed = %d must be in [0, 2^64)" % seed)
    return seed


def _device(device=None):
    """``device`` as a torch.device; None: the default device."""
    return torch.device(default_device() if device is None else device)


# (with a scalar, one tangent) -> (workspace query, step) of a tangent step: PeriodicSolver._launch_tangent
_TANGENT_STEPS = {(False, True): (ops.spec_ns_tangent_workspace, ops.spec_ns_step_tangent_),
                  (True, True): (ops.spec_ns_scalar_tangent_workspace, ops.spec_ns_step_scalar_tangent_),
                  (False, False): (ops.spec_ns_tangents_workspace, ops.spec_ns_step_tangents_),
                  (True, False): (ops.spec_ns_scalar_tangents_workspace, ops.spec_ns_step_scalar_tangents_)}

Diagnostics = collections.namedtuple('Diagnostics', ['energy', 'enstrophy', 'power_in'])
ScalarDiagnostics = collections.namedtuple('ScalarDiagnostics', ['variance', 'dissipation', 'flux_x', 'flux_y'])
Spectrum = collections.namedtuple('Spectrum', ['k', 'energy', 'enstrophy', 'injection', 'variance'])
Transfer = collections.namedtuple('Transfer', ['k', 'energy', 'enstrophy', 'variance'])
LinearRates = collections.namedtuple('LinearRates', ['k', 'energy', 'enstrophy'])


def flux(t):
    """The spectral flux Pi(s) = -sum_{s' <= s} T(s') of a transfer T [..., S] (a field of ``Transfer``): the rate at which the nonlinear term
    carries the quantity out of the shells <= s, positive for a cascade towards small scales; Pi(S - 1) = 0 to rounding."""
    return -torch.cumsum(t, dim=-1)


def kaplan_yorke_dimension(exponents):
    """The Kaplan-Yorke (Lyapunov) dimension of a spectrum of exponents [..., K] (a torch tensor; it stays on its device), over the last
    axis: with the exponents sorted descending and S_j the sum of the first j, j the largest count with S_j >= 0, it is j + S_j / |lambda_(j+1)|.
    0 where the leading exponent is negative.  K where every partial sum is >= 0: the K exponents given do not reach the point where the
    volume contracts, so K is then only a LOWER BOUND of the dimension -- compute more exponents.  nan where an exponent is nan."""
    lam = torch.sort(exponents, dim=-1, descending=True).values
    K = lam.shape[-1]
    S = torch.cumsum(lam, dim=-1)
    count = torch.arange(1, K + 1, device=lam.device)
    j = torch.amax(torch.where(S >= 0, count, torch.zeros_like(count)), dim=-1, keepdim=True)            # S_j >= 0 holds on a prefix
    zero = torch.zeros_like(lam[..., :1])
    Sj = torch.gather(torch.cat([zero, S], dim=-1), -1, j)                                               # S_0 = 0
    nxt = torch.gather(torch.cat([lam, torch.ones_like(zero)], dim=-1), -1, j)                           # lambda_(j+1); unused at j = K
    dim = torch.where(j == K, j.to(lam.dtype), j.to(lam.dtype) + Sj / nxt.abs())
    return torch.where(torch.isnan(lam).any(dim=-1, keepdim=True), torch.full_like(dim, float('nan')), dim)[..., 0]


class PeriodicState(object):
    """State of a PeriodicSolver run; owns its device buffers.
    what: the vorticity spectrum, compacted to the kept y-wavenumbers and transposed (float32 [B, my1, nx, 2], include/nns.h: nns_spec_ns_*);
    mean: the conserved mean velocity (U0, V0) per grid, float32 [B, 2]; work: the solver's scratch; steps: steps taken since init;
    that: the passive scalar's spectrum in the layout of what, its (0, 0) mode (the mean of the scalar) kept, or None without a scalar;
    clock: int64 [1] on the device, the stochastic steps taken (the step index of the next kick; the step advances it on the device, so a
    captured step replays); noise_ids: int32 [B] on the device, the grid ids of the noise (default arange(B): grids with equal ids get equal
    noise, and a single grid with id k repeats member k of a batch).  Both None until a stochastic step needs them."""

    def __init__(self, what, mean, work, that=None, clock=None, noise_ids=None):
        self.what, self.mean, self.work, self.that = what, mean, work, that
        self.clock, self.noise_ids = clock, noise_ids
        self.steps = 0

    @property
    def batch(self):
        return self.what.shape[0]

    def clone(self):
        """A copy with its own buffers (a fresh workspace: the solver keeps no data in it between calls)."""
        copy = lambda t: None if t is None else t.clone()
        c = PeriodicState(self.what.clone(), self.mean.clone(), torch.empty_like(self.work), copy(self.that), copy(self.clock), copy(self.noise_ids))
        c.steps = self.steps
        return c


class PeriodicParticles(object):
    """Lagrangian tracers of a PeriodicSolver (``init_particles``); owns its device buffers.
    pos: float64 [B, P, 2] = (x, y) on the device, UNWRAPPED (``wrapped()`` folds them into the box; mean-square displacement needs them as
    they are); order: 4 (cubic) or 6 (quintic B-splines).  Private: two sets of (u, v) spline coefficients (float32 [2, B, nx, ny]: the flow
    at two step boundaries), the Runge-Kutta accumulator and stage position (float64 [B, P, 2]) and the coefficient build's workspace, all
    made here so that ``advect`` allocates nothing."""

    def __init__(self, pos, order, box, grid):
        self.pos, self.order, self.box, self.grid = pos, order, box, grid
        B, dev = pos.shape[0], pos.device
        self._coef = tuple(torch.empty((2, B) + tuple(grid), dtype=torch.float32, device=dev) for _ in range(2))
        self._acc, self._stage = torch.empty_like(pos), torch.empty_like(pos)
        self._work = torch.empty(ops.spec_ns_particle_workspace(B, 2, *grid), dtype=torch.uint8, device=dev)

    @property
    def batch(self):
        return self.pos.shape[0]

    @property
    def count(self):
        return self.pos.shape[1]

    def clone(self):
        """A copy with its own buffers (nothing is kept in the private ones between calls)."""
        return PeriodicParticles(self.pos.clone(), self.order, self.box, self.grid)

    def wrapped(self):
        """The positions folded into the box [0, Lx) x [0, Ly): a new float64 [B, P, 2] tensor."""
        L = torch.tensor(self.box, dtype=torch.float64, device=self.pos.device)
        return self.pos - L * torch.floor(self.pos / L)


_Run = collections.namedtuple('_Run', ['solver', 'nsteps', 'mean', 'velocity', 'scalar', 'noise'])        # the constants of one _AdvanceFn call


class _AdvanceFn(torch.autograd.Function):
    """``PeriodicSolver.evolve`` / ``evolve_velocity`` and ``advance*`` as one autograd node.  Inputs: ``run``, the call's constants (a
    ``_Run``), then what the call is differentiable in: ``forcing`` (or None), ``operator`` (or None) and the ``fields``, (w,) or (u0, v0),
    then with ``run.scalar`` theta.  Forward: the step the solver's own ``_launch_steps`` takes on a fresh state, with the spectra at the start
    of every step kept (one device copy each between one-step calls: the step itself is untouched).  Backward: ops.spec_ns_adjoint_ between
    the compact and expand kernels.  A stochastic step has no adjoint of its own: the kick is additive and independent of the state, the
    saved start spectra carry it, and the generator is never run in the backward.  ``run.noise``: (clock, noise_ids) of ``evolve`` for the
    state the forward steps (ignored without a stochastic force).  ``operator``: the table of ``evolve`` that takes the solver's place: the
    step is then the linear one, and where the table requires grad the adjoint also sums the table's cotangent per grid, which
    ``_operator_gradient`` turns into the table's gradient.  ``run.velocity``: the flow's ends are init / fields instead of the vorticity's;
    theta's are spec_ns_scalar_init / spec_ns_scalar_field."""

    @staticmethod
    def forward(ctx, run, forcing, operator, *fields):
        s, nsteps, mean, velocity, scalar, noise = run
        theta = fields[-1].detach() if scalar else None
        if velocity:
            state = s.init(fields[0].detach(), fields[1].detach(), theta)
        else:
            state = s.init_vorticity(fields[0].detach(), mean)
            if scalar:
                state.that = ops.spec_ns_scalar_init(s._field('theta', theta).contiguous(), torch.empty_like(state.what), state.work)
        ghat = s._force_of(state) if forcing is None else s._source_spectrum(forcing.detach(), state)
        what0 = torch.empty((nsteps,) + tuple(state.what.shape), dtype=torch.float32, device=state.what.device)
        that0 = torch.empty_like(what0) if scalar else None
        if s.stoch_amp is not None:
            state.clock, state.noise_ids = s._noise_args(noise[0], noise[1], state)
        if operator is None:
            lin = s._linear_of(state) if s._linear() else None
        else:
            lin = s._operator_of(operator, state)
        for k in range(nsteps):
            what0[k].copy_(state.what)
            if scalar:
                that0[k].copy_(state.that)
            s._launch_steps(state, 1, ghat, lin)
        ctx.run, ctx.lin, ctx.squeeze = run, lin, fields[0].dim() == 2
        ctx.shared = forcing is not None and forcing.shape[0] == 1 and state.batch > 1
        ctx.force_shape = None if forcing is None else tuple(forcing.shape)
        ctx.save_for_backward(what0, state.mean, *(t for t in (that0, ghat) if t is not None))
        out = s.fields(state)[:2] if velocity else (s.vorticity(state),)
        if scalar:
            out = tuple(out) + (s.scalar(state),)
        return tuple(o[0] for o in out) if ctx.squeeze else tuple(out)

    @staticmethod
    def backward(ctx, *gout):
        s, velocity, scalar = ctx.run.solver, ctx.run.velocity, ctx.run.scalar
        _, need_g, need_l = ctx.needs_input_grad[:3]                         # of forward's run, forcing, operator
        what0, mean = ctx.saved_tensors[:2]
        rest = list(ctx.saved_tensors[2:])
        that0 = rest.pop(0) if scalar else None
        ghat = rest[0] if rest else None
        B, dev = what0.shape[1], what0.device
        shape = (B, s.nx, s.ny)
        gout = [torch.zeros(shape, dtype=torch.float32, device=dev) if g is None else g.reshape(shape).contiguous() for g in gout]
        work = s._work(ops.spec_ns_scalar_adjoint_workspace if scalar else ops.spec_ns_adjoint_workspace, B, dev)
        if velocity:                                      # K^T (ubar, vbar)^ = curl(ubar, vbar)^ / |k|^2
            lam = s.init(gout[0], gout[1]).what * s._k2_table(dev, -1)
        else:
            lam = s.init_vorticity(gout[0]).what
        gbar = torch.empty_like(lam) if need_g else None
        mu = ops.spec_ns_scalar_init(gout[-1], torch.empty_like(lam), work) if scalar else None
        lbar = torch.empty_like(lam) if need_l else None
        ops.spec_ns_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa if scalar else 0.0,
                             s.scalar_gradient, s.buoyancy, ctx.lin, lbar)
        if velocity:                                      # init^T (lam) = (lam_y, -lam_x): the velocity of the streamfunction lam
            grads = tuple(s.fields(s._at_rest(lam * s._k2_table(dev, 1), work))[:2])
        else:
            grads = (s.vorticity(s._at_rest(lam, work)),)
        if scalar:
            grads = grads + (ops.spec_ns_scalar_field(mu, work, s.ny),)
        if ctx.squeeze:
            grads = tuple(g[0] for g in grads)
        gf = None
        if need_g:
            gf = s.vorticity(s._at_rest(gbar, work))
            if ctx.shared:
                gf = torch.sum(gf, dim=0, keepdim=True)
            gf = gf.reshape(ctx.force_shape)
        gop = None if lbar is None else s._operator_gradient(lbar)
        return (None, gf, gop) + grads


_Look = collections.namedtuple('_Look', ['solver', 'fields', 'mean', 'order'])        # the constants of one _ObserveFn call


class _ObserveFn(torch.autograd.Function):
    """``PeriodicSolver.observe`` as one autograd node.  Inputs: ``look``, the call's constants (a ``_Look``), then what the call is
    differentiable in: the vorticity field w, theta (or None) and the positions x, y (float64 [B, P] or [P]).  Forward: ``sample``'s own
    calls on ``init_vorticity(w, mean)`` with the scalar set as ``_AdvanceFn.forward`` sets it.  Backward into w and theta: the particles'
    cells, the sort, the spread (the gather's transpose, no atomics), the coefficient build's transpose, then ``vorticity`` /
    ``spec_ns_scalar_field`` as the ends of ``_AdvanceFn.backward``.  Backward into x and y: the cotangent times the spline's derivative at
    the particle, summed over the fields in float64; for that the forward keeps the coefficient images or, where they are smaller, the
    spectra (and builds the images again).  A branch that nobody asked for launches nothing."""

    @staticmethod
    def forward(ctx, look, w, theta, x, y):
        s, fields, mean, order = look
        state = s.init_vorticity(w.detach(), mean)
        if theta is not None:
            state.that = ops.spec_ns_scalar_init(s._field('theta', theta.detach()).contiguous(), torch.empty_like(state.what), state.work)
        shared = x.dim() == 1
        p = s.init_particles(x.detach(), y.detach(), order, batch=state.batch if shared else None)
        s._particles(p, state)
        mask, slots = s._field_mask(fields, state)
        coef = s._coefficients(state, mask, order)
        out = ops.spec_ns_particle_sample(coef, p.pos, order, s.Lx, s.Ly)
        ctx.look, ctx.mask, ctx.slots, ctx.shared, ctx.wshape = look, mask, slots, shared, tuple(w.shape)
        ctx.kept = None
        keep = [p.pos]
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            spectra = (1 if mask & 7 else 0) + (1 if mask & 8 else 0)
            if spectra * s.my1 * 8 < len(set(slots)) * s.ny * 4:          # bytes per grid row: compact spectra against coefficient images
                ctx.kept = 'spectra'
                keep += [state.what, state.mean] + ([state.that] if mask & 8 else [])
            else:
                ctx.kept = 'coef'
                keep.append(coef)
        ctx.save_for_backward(*keep)
        return out if slots == list(range(out.shape[-1])) else out[..., slots].contiguous()

    @staticmethod
    def backward(ctx, gout):
        s, order = ctx.look.solver, ctx.look.order
        mask, slots = ctx.mask, ctx.slots
        need_w, need_t, need_x, need_y = ctx.needs_input_grad[1:]
        pos = ctx.saved_tensors[0]
        B, P, dev = pos.shape[0], pos.shape[1], pos.device
        nf = bin(mask).count('1')
        gout = gout.to(torch.float32)
        if slots == list(range(nf)):
            cot = gout.contiguous()
        else:                                             # a field named twice, or out of the mask's order: sum into the mask's slots
            cot = torch.zeros((B, P, nf), dtype=torch.float32, device=dev).index_add_(2, torch.tensor(slots, device=dev), gout)
        wbar = thbar = xbar = ybar = None
        if (need_w and mask & 7) or (need_t and mask & 8):
            perm, start = ops.spec_ns_particle_cells(pos, s.nx, s.ny, s.Lx, s.Ly)
            cbar = ops.spec_ns_particle_spread(cot, pos, perm, start, s.nx, s.ny, order, s.Lx, s.Ly)
            wbar_hat, thbar_hat = ops.spec_ns_particle_coefs_adjoint(cbar, mask, order, s.Lx, s.Ly)
            work = s._work(ops.spec_ns_scalar_workspace, B, dev)
            if need_w and mask & 7:
                wbar = s.vorticity(s._at_rest(wbar_hat, work)).reshape(ctx.wshape)
            if need_t and mask & 8:
                thbar = ops.spec_ns_scalar_field(thbar_hat, work, s.ny).reshape(ctx.wshape)
        if need_x or need_y:
            if ctx.kept == 'coef':
                coef = ctx.saved_tensors[1]
            else:
                what, mean = ctx.saved_tensors[1:3]
                state = PeriodicState(what, mean, s._work(ops.spec_ns_workspace, B, dev), ctx.saved_tensors[3] if mask & 8 else None)
                coef = s._coefficients(state, mask, order)
            grad = ops.spec_ns_particle_sample_grad(coef, pos, order, s.Lx, s.Ly)
            pbar = torch.sum(cot.to(torch.float64).unsqueeze(-1) * grad.to(torch.float64), dim=2)          # [B, P, 2]
            if ctx.shared:
                pbar = torch.sum(pbar, dim=0)
            xbar = pbar[..., 0].contiguous() if need_x else None
            ybar = pbar[..., 1].contiguous() if need_y else None
        return None, wbar, thbar, xbar, ybar


SecondOrderGradients = collections.namedtuple('SecondOrderGradients', ['wbar', 'dwbar', 'gbar', 'dgbar'])


class SecondOrderRun(object):
    """What ``PeriodicSolver.second_order_forward`` returns: ``w`` and ``dw``, the vorticity field and its perturbation after the steps
    (bitwise ``evolve``'s forward and ``evolve_tangent``'s), and the spectra (w^, dw^) at the start of every step, kept for ``backward``
    (``what0``, ``dwhat0``: float32 [nsteps, B, my1, nx, 2] each).  ``backward`` may be called any number of times."""

    def __init__(self, solver, fields, what0, dwhat0, mean, ghat, dghat, lin, force_shape, squeeze):
        self.solver, (self.w, self.dw) = solver, fields
        self.what0, self.dwhat0, self.mean, self.ghat, self.dghat, self.lin = what0, dwhat0, mean, ghat, dghat, lin
        self.force_shape, self.squeeze = force_shape, squeeze

    def backward(self, lam, dlam):
        """``SecondOrderGradients(wbar, dwbar, gbar, dgbar)``, fields like ``w``: for the cotangent ``lam`` of ``w`` and its derivative
        ``dlam`` in the direction the run carries, wbar = J^T lam and gbar, the gradients in the initial field and in ``forcing``, bitwise the
        backward of ``evolve``; dwbar and dgbar their derivatives in the direction (dw, dforcing, dlam): the second-order adjoint of the
        Lawson RK4 step as HIP kernels, 16 launches per step (include/nns.h: nns_spec_ns_step_second_adjoint_f32).  gbar and dgbar are None
        for a run without ``forcing``, and summed over the batch (one deterministic torch.sum each) for a shared one."""
        s = self.solver
        B, dev = self.what0.shape[1], self.what0.device
        shape = (B, s.nx, s.ny)
        spectra = []
        for name, f in (('lam', lam), ('dlam', dlam)):
            f = s._field(name, f.detach() if isinstance(f, torch.Tensor) else f).to(dev)
            if tuple(f.shape) != shape:
                raise ValueError("backward: %s must be %s like the run's fields, got %s" % (name, list(shape), tuple(f.shape)))
            spectra.append(s.init_vorticity(f.contiguous()).what)
        lamh, dlamh = spectra
        work = s._work(ops.spec_ns_second_adjoint_workspace, B, dev)
        need_g = self.force_shape is not None
        gbar = torch.empty_like(lamh) if need_g else None
        dgbar = torch.empty_like(lamh) if need_g else None
        ops.spec_ns_second_adjoint_(self.what0, self.dwhat0, self.mean, self.ghat, self.dghat, lamh, dlamh, gbar, dgbar, work, s.ny, s.Lx, s.Ly,
                                    s.dt, s.nu, s.drag, self.lin)
        out = [s.vorticity(s._at_rest(lamh, work)), s.vorticity(s._at_rest(dlamh, work))]
        if self.squeeze:
            out = [o[0] for o in out]
        for g in (gbar, dgbar):
            if g is not None:
                g = s.vorticity(s._at_rest(g, work))
                if self.force_shape[0] == 1 and B > 1:
                    g = torch.sum(g, dim=0, keepdim=True)
                g = g.reshape(self.force_shape)
            out.append(g)
        return SecondOrderGradients(*out)


class PeriodicSolver(object):
    """Batched 2-D incompressible Navier-Stokes on the periodic box [0, Lx) x [0, Ly): float32 fields [B, nx, ny] on the device
    (axis 0 = x), nx and ny each a power of two in [64, 1024].  Vorticity-streamfunction form, 2/3-rule dealiasing
    (3|m_x| < nx and 3|m_y| < ny), integrating-factor (Lawson) RK4 in time; every step is HIP (csrc/pspec_kernels.hip), no FFT library.

    ``init(u, v)`` PROJECTS the input: the state keeps the vorticity of (u, v) inside the 2/3 band and the grid means (U0, V0), so
    ``fields(init(u, v))`` returns the divergence-free, band-limited part of (u, v) -- equal to it when (u, v) already is one.
    The mean velocity is conserved.  ``p`` is the pressure of the velocity field: lap p = 2 rho (u_x v_y - u_y v_x), zero mean.

    Forcing and drag: with ``set_forcing(fx, fy)`` (a force constant in time) and ``drag`` = alpha >= 0 the solver integrates
        u_t + (u . grad) u = -grad p / rho + nu lap u - alpha (u - <u>) + f_s
    where <.> is the grid mean and f_s the solenoidal, zero-mean, band-limited part of f (``forcing_fields()``): a gradient part of f only
    shifts the pressure and a mean part only accelerates the frame, so both are dropped, as ``init`` drops them from a velocity.  The mean
    velocity stays conserved and undamped and ``p`` keeps its definition (div f_s = 0).  ``diagnostics(state)`` gives energy, enstrophy and
    the power input of the force per grid.  Without a force and with drag == 0 every call takes the unforced path.

    Passive scalar: with ``kappa`` >= 0 (None: no scalar) and ``init(u, v, theta)`` the state also carries a scalar theta -- temperature,
    dye, concentration -- that the flow advects and that, without ``buoyancy``, does not act back on it:
        theta_t + (u . grad) theta = kappa lap theta - G . u
    ``scalar_gradient`` = G = (Gx, Gy) is a uniform mean gradient: the total field is G . x + theta and theta its periodic part, whose variance
    the gradient sustains.  theta is band-limited like the flow but keeps its grid mean, d<theta>/dt = -G . (U0, V0); the drag does not act
    on it.  It rides in the flow's launches (still 8 per step), each RK stage with that stage's own velocity, and the flow evolves bitwise
    as without it.  ``scalar(state)`` gives theta, ``scalar_diagnostics(state)`` its variance budget.  A state without a scalar takes exactly
    the calls it takes on a solver without ``kappa``.

    Buoyancy: with ``buoyancy`` = b = (bx, by) != 0 (needs ``kappa``) the scalar of a state acts on its flow (Boussinesq):
        u_t + (u . grad) u = -grad p / rho + nu lap u - alpha (u - <u>) + f_s + b theta',      theta' = theta - <theta>
    that is w_t gains by theta_x - bx theta_y, explicit in the same Lawson RK4 with every stage's own theta^, still 8 launches per step.  Only the
    periodic fluctuation is buoyant: b <theta> would only accelerate the frame, and the background G . x is taken as hydrostatic (its curl, a
    constant, cannot exist on a periodic box), so both are dropped, as ``init`` and ``set_forcing`` drop such parts.  b . G > 0 gives internal
    gravity waves and stratified turbulence, b . G < 0 homogeneous Rayleigh-Benard convection.  Now div(b theta') != 0 and ``fields`` returns the
    pressure of lap p = rho (2 (u_x v_y - u_y v_x) + b . grad theta).  ``buoyancy_power(state)`` = b . <u theta'> closes the energy equation,
    d energy / dt = power_in - 2 nu enstrophy - 2 drag energy + buoyancy_power; ``buoyancy_spectrum(state)`` gives it per shell and
    ``energy_budget`` adds it.  With b = (0, 0), and for a state without a scalar (theta = 0), every call is the one it is without the argument.

    Stochastic forcing: ``set_stochastic_forcing(rate_by_shell, seed)`` (or ``ring_forcing``) adds a Gaussian force, white in time, on the modes of
    chosen shells: after every complete deterministic step n (drag, steady force, scalar and buoyancy included, whichever are active)
        w^_k <- w^_k + sqrt(dt) a_k xi_k(n, id)         E |xi|^2 = 1, independent over modes, steps and grid ids
    with xi from a counter-based generator (Philox4x32-10, keyed by ``seed``) evaluated inside the step's last launch: still 8 launches per
    step, capturable, and the eager loop, one call of many steps and graph replay give the same bits.  The noise is additive, so there is no
    Ito / Stratonovich ambiguity, and the MEAN energy input per shell is known in advance and independent of the state
    (``stochastic_injection``).  ``state.clock`` counts the steps on the device and ``state.noise_ids`` names the noise of every grid.  The
    scalar gets no noise.  ``_forced()``, ``diagnostics().power_in`` and ``spectrum().injection`` keep their meaning: the STEADY force only.
    Without a stochastic force every call is the one it is without this feature.

    Linear operator: ``hyperviscosity`` = (nu_h, p), ``hypofriction`` = (mu, q) and ``beta`` add the three standard linear terms of forced 2-D and
    geophysical turbulence to the vorticity equation,
        w_t + u w_x + v w_y + beta v' = nu lap w - nu_h (-lap)^p w - drag w - mu (-lap)^-q w + g + (buoyancy) + (noise),      v' = v - <v>
    (beta <v> would be a constant source in the (0, 0) mode, which the periodic box cannot hold: it is dropped, as ``init`` and ``set_forcing``
    drop such parts, and the mean velocity stays conserved).  All three are diagonal in Fourier space: mode k has
        lambda_k = -(nu |k|^2 + drag + nu_h |k|^2p + mu |k|^-2q) + i beta kx / |k|^2,        lambda_(0,0) = 0       (``linear_operator()``)
    and the Lawson RK4 integrates it exactly with the complex factors exp(lambda dt / 2), exp(lambda dt): no stiffness limit on nu_h K^2p dt or
    beta dt / k, no further launch (still 8 per step) or transform.  A plane wave is an exact solution: a Rossby wave of frequency
    -beta kx / |k|^2 (westward) and amplitude exp(Re(lambda) t).  The scalar keeps its operator kappa |k|^2.  The step reads lambda dt / 2 from
    a float32 table made at construction from the arguments as they are then, shared by the batch.  ``linear_spectrum(state)`` gives the
    linear term's energy and enstrophy rates per shell (beta contributes to neither) and ``energy_budget`` uses it.  With nu_h = 0, mu = 0 and
    beta = 0 every call is the one it is without these arguments.

    Reverse mode: ``evolve(w, nsteps, theta=, mean=, forcing=, clock=, noise_ids=)`` and ``evolve_velocity`` advance fields through ``nsteps``
    steps of ANY solver as one autograd node, differentiable in the initial fields and in a vorticity source ``forcing``: the forward is bitwise
    ``step``, the backward the adjoint of the Lawson RK4 step as HIP kernels, 16 launches per step.  The linear operator above is transposed
    exactly: under the grid sum that pairs cotangents the transpose of the factor E_k = exp(lambda_k dt / 2) is conj(E_k), read from the same
    table.  A stochastic step is differentiated as the deterministic step it contains -- the kick is additive and independent of the state, so
    its Jacobian is the identity and the saved start spectra carry it; ``clock`` names the first step's noise, so a rollout cut into chunks
    repeats the uncut noise.  Both also take ``operator``, a table (Re, Im)(lambda_k dt / 2) in the step's own layout that replaces the solver's
    linear operator for the call and in which the call is differentiable too: for E = exp(l) the stages' derivatives in l need no N and no
    division by E (d s1 = s1, d s2 = E w0, d s3 = s3 + E^2 w0, d w1 = (s3 + E^2 w0) / 3 + 2/3 E (s1 + s2)), and the adjoint's stages 3-1 sum
    their products with the cotangents they already hold, in the same 16 launches (tests/pspec_operator_grad_oracle.py).  That covers nu, drag,
    nu_h, mu and beta through ``operator_table`` and any learned diagonal operator, a per-mode eddy viscosity nu(k) for one, through
    ``mode_table``.  With ``operator`` the call takes the LINEAR form of the step also on a solver without hyperviscosity, hypofriction or
    beta: with a table of nu and drag alone that is the forced step's mathematics but not bitwise the forced step.  kappa, G, b, the noise
    amplitudes, the seed, the mean flow and per-grid operators stay constants; ``advance*`` do not take the argument.  ``advance``,
    ``advance_velocity``, ``advance_scalar`` and ``advance_velocity_scalar`` are the same node on the solvers they were written for (the
    steady-forced flow; with ``kappa``, its scalar and buoyancy) and refuse the others.

    Forward mode: ``step_tangent(state, dwhat, nsteps, dforcing=)`` advances the state exactly as ``step`` does -- bitwise, on the plain,
    forced, linear and stochastic solvers -- and with it a perturbation spectrum dwhat, which comes out as J dwhat, J the Jacobian of those
    steps: where the reverse mode gives J^T r, this gives J d, and sum(J d . r) = sum(d . J^T r) ties the two sets of kernels together at
    float32 round-off.  The Lawson RK4 recurrences are linear in (w^, N^), so the tangent step is the same four stages on d with the same
    factors E (drag, hyperviscosity, hypofriction and beta act through them) and dN_i = -M [u d_x + v d_y + du w_x + dv w_y]^ + dg^, u, v,
    w_x, w_y those of stage i's own state.  The perturbation rides in the step's launches as the scalar does (still 8 per step,
    capturable), has no mean flow and no (0, 0) mode, and gets no kick: the noise is a constant of the call.  Nothing is stored per step
    (the adjoint keeps a spectrum per step).  ``evolve_tangent`` / ``evolve_velocity_tangent`` are the field-level forms, ``evolve``'s
    forward bitwise; ``lyapunov_exponent`` the leading finite-time exponent in the energy norm.  Several tangents sharing one base:
    ``step_tangents(state, dwhat, nsteps)`` carries K <= 32 perturbations dwhat [K, B, my1, nx, 2] (``init_tangents``) in one call, the state
    bitwise as by ``step`` and every dwhat[k] bitwise as by ``step_tangent`` alone; u, v, w_x, w_y of a stage are transformed once for all
    K, so the y-transforms and the passes through a column tile tend to one half of K separate calls' (still 8 launches per step).
    ``tangent_gram`` is their Gram matrix in the energy inner product, ``orthonormalize_tangents`` a Cholesky QR done twice (Gram and
    recombination in HIP, the K x K algebra in torch float64 on the device), ``lyapunov_spectrum`` the first K finite-time exponents with
    the backward Lyapunov vectors left in dwhat, and the module's ``kaplan_yorke_dimension`` the attractor's dimension from them.
    With a scalar (passive or Boussinesq) the perturbation is the pair (dw^, dtheta^) of the one system, under names of its own as
    ``advance_scalar`` stands beside ``advance``: ``step_tangent_scalar(state, dwhat, dthat, nsteps, dforcing=)`` advances (what, that)
    bitwise as ``step`` does -- passive, buoyant, linear or stochastic -- and the pair by the Jacobian of those steps, with
    dN_w = -M [u dw_x + v dw_y + du w_x + dv w_y]^ + dg^ + M (i kx by - i ky bx) dtheta^ and
    dN_theta = -M_theta [u dtheta_x + v dtheta_y + du (theta_x + Gx) + dv (theta_y + Gy)]^ about every stage's own state; dw^ takes the
    vorticity's factors, dtheta^ the scalar's real E_theta and keeps its (0, 0) mode, which is carried unchanged and acts on nothing
    (tests/pspec_scalar_tangent_oracle.py).  The pair rides in the scalar step's launches (still 8 per step).  ``evolve_tangent_scalar`` /
    ``evolve_velocity_tangent_scalar`` are the field-level forms, ``lyapunov_exponent_scalar`` the leading exponent in the norm
    E(dw) + scalar_weight 1/2 <dtheta'^2>.  K pairs on one base with a scalar: ``step_tangents_scalar(state, dwhat, dthat, nsteps)`` carries
    K <= 32 pairs [K, B, my1, nx, 2] (``init_tangents_scalar``), the state bitwise as by ``step`` and every pair bitwise as by
    ``step_tangent_scalar`` alone, the base's three inverse and two forward y-transforms and its two passes through a column tile done once
    for all K; ``tangent_gram_scalar`` is the Gram matrix in that norm (the energy Gram of dwhat + scalar_weight times the variance Gram of
    dthat, both float64 HIP), ``orthonormalize_tangents_scalar`` the same Cholesky QR done twice on the pair and
    ``lyapunov_spectrum_scalar`` the first K exponents (tests/pspec_scalar_lyapunov_oracle.py); ``kaplan_yorke_dimension`` applies.
    ``step_tangent``, ``lyapunov_exponent``, ``step_tangents`` and ``lyapunov_spectrum`` keep refusing
    a state that carries a scalar.  Not built: the
    tangent in ``operator``, a source perturbation per tangent, covariant vectors, and a ``jvp`` hook on the autograd node for
    ``torch.autograd.forward_ad``.

    Second order: ``hessian_vector_product(loss, w, dw, nsteps, forcing=, dforcing=)`` gives the value, the gradient and the exact
    Hessian-vector product of a loss of the rollout, jointly in the initial vorticity and the source -- what Newton-CG, trust-region 4D-Var,
    Hessian eigenvalues and second-order sensitivities need, and what a Gauss-Newton product J^T J d (``evolve_tangent`` then the backward
    of ``evolve``) leaves out: sum lam . d^2 Phi[d, .].  It is reverse mode through the tangent.  The nonlinear term is bilinear, so
    N'(s)^T kappa is linear in s and the derivative of an adjoint stage in the direction d is the same operator about the TANGENT stage
    state, without the mean flow: dr = N'(s_i)^T dkappa + N'_0(d_i)^T kappa, and (dlam, dkappa, dwbar, dgbar) obey the adjoint's own linear
    recurrences (tests/pspec_second_adjoint_oracle.py).  ``second_order_forward`` is ``evolve_tangent`` with (w^, dw^) kept per step
    (16 bytes per stored mode), and its run's ``backward(lam, dlam)`` recomputes the stages of both by the tangent step's launches and carries
    the second quadruple through the adjoint's: still 16 launches per step, the first-order outputs bitwise those of ``evolve``.  Plain,
    forced, linear and stochastic solvers (a stochastic step is differentiated as the deterministic step it contains).  Not built: the
    scalar and Boussinesq system (a solver with ``kappa`` is refused), the second derivative in ``operator``, velocity-level ends, K
    directions sharing one base.

    By wavenumber: the stored modes are binned into shells of width dk = min(2 pi / Lx, 2 pi / Ly) centred on k_s = s dk (``shells()``; an
    elongated box has many).  ``spectrum(state)`` gives energy E(s), enstrophy Z(s), the force's injection F(s) and the scalar's variance V(s),
    whose sums over the shells are the numbers of ``diagnostics`` and ``scalar_diagnostics``; ``transfer(state)`` the nonlinear transfers T(s)
    of energy, enstrophy and scalar variance from one evaluation of the step's own dealiased nonlinear term (each sums to zero), ``flux`` their
    cumulative form Pi(s), and ``energy_budget(state)`` dE(s)/dt = T_E + F - 2 nu Z - 2 drag E (T_E + F + D_E with the general linear operator).  All float64, summed on the device in a fixed
    order.  The spectrum of arbitrary fields -- a model's prediction, say -- is ``solver.spectrum(solver.init(u, v))``.

    Lagrangian tracers: ``init_particles(x, y, order=4)`` makes ``PeriodicParticles`` (float64 positions [B, P, 2] on the device, unwrapped:
    only the cell index is taken modulo the box), ``sample(state, particles, fields=('u', 'v'))`` reads u, v, the vorticity 'w' and 'theta' at
    them, and ``advect(state, particles, nsteps, scheme='rk4')`` carries them with the flow while it steps the state, bitwise as ``step`` does
    (csrc/pspec_particles.hip, tests/pspec_particles_oracle.py).  Reads are periodic tensor-product B-splines of order 4 (cubic, 4 x 4 nodes)
    or 6 (quintic, 6 x 6) whose prefilter is done exactly in Fourier space, where the solver already is: the coefficients of a field are
    irfft2(f^ / (beta_x beta_y)), beta the spline's symbol (>= 0.5 / 0.325 inside the 2/3 band), the mean flow in the (0, 0) coefficient --
    one pointwise launch and one inverse transform, ``fields`` without its pressure solve (``particle_coefficients`` hands the images out).
    Against the exact Fourier sum a field with |m| <= 8 is read to 4.3e-4 (order 4) and 6.7e-6 (order 6) of its maximum at 64^2 and to
    2.7e-5 and 9.6e-8 at 128^2; a white spectrum up to the band's edge, 1.5 points per half wavelength, is the honest limit of a 4- or
    6-point stencil: 3-4 % and 0.6-0.8 % (two draws at 64^2).  The gather kernel has one lane per particle, cell and offset in float64, weights in float32 registers,
    a fixed order of summation, no atomics: a particle's values depend on its own position and its grid alone and repeat bitwise.  Time
    stepping: classical RK4 with step 2 dt over a PAIR of flow steps, k1 = U_n(x), k2 = U_n+1(x + dt k1), k3 = U_n+1(x + dt k2),
    k4 = U_n+2(x + 2 dt k3), x <- x + dt/3 (k1 + 2 k2 + 2 k3 + k4) -- U at the step boundaries is exactly what the Lawson RK4 flow gives,
    so there is no interpolation in time and no change to the step (``nsteps`` even); ``scheme='heun'`` (x* = x + dt U_n(x),
    x <- x + dt/2 (U_n(x) + U_n+1(x*))) takes any ``nsteps``.  Velocities are float32 from the kernel, the position update float64.  One
    coefficient build and two particle launches per flow step, no allocation, no host synchronisation, capturable; n steps in one call are
    bitwise n / 2 calls of 2.  Both schemes work on every solver, since they read (w^, mean) at step boundaries only; under stochastic forcing
    the flow is not smooth in time and the formal order in time is lost.  Not built: inertial particles, several GPUs.

    Observations at points, differentiable: ``observe(w, x, y, fields=('u', 'v'), theta=, mean=, order=4)`` is ``sample`` as one autograd
    node -- forward bitwise ``sample(init_vorticity(w, mean), init_particles(x, y, order), fields)`` -- so that
    ``loss(observe(evolve(w0, n), x, y))`` back-propagates into w0, theta0, the forcing and the operator table through ``evolve``, and
    into the float64 positions (csrc/pspec_particles.hip, tests/pspec_particles_adjoint_oracle.py).  The backward into the fields is the
    transpose of sample's chain, link by link.  The gather's transpose is a scatter, written as a gather without floating-point atomics:
    ``particle_cells`` keys every particle by the wrapped cell the gather finds it in and sorts stably on the device (no host
    synchronisation); a staging launch writes one record per sorted slot (the forward's float64 weights, rounded once, and the
    cotangents); a node launch sums, for every node, the particles of the order x order cells whose stencil covers it -- a ascending, c
    ascending, the cell's slots ascending, wx[a] wy[c] one float32 multiply, every term one float64 fma, one rounding on store.  It repeats
    bitwise, a grid does not depend on its batch neighbours, and nodes no particle reaches are exact zeros; ``spread(particles, values)``
    hands it out (point forces, binning).  The coefficient build's transpose is its Fourier multipliers conjugated,
    wbar^ = M [(-i ky c_u^ + i kx c_v^) / |k|^2 + c_w^] / (beta_x beta_y) with (0, 0) zero, thetabar^ = M c_theta^ / (beta_x beta_y), after one
    forward transform per field; ``vorticity`` / ``scalar`` then give the fields' cotangents.  The backward into the positions is the
    cotangent times the spline's own derivative, ``sample_gradient(state, particles, fields)`` = float32 [B, P, nf, 2]: the gather with
    derivative weights on one axis -- for (u, v) the velocity-gradient tensor at the particle (strain, Okubo-Weiss, FTLE along
    trajectories).  It differences neighbouring float32 coefficients over h, so on a fine axis it carries their transform error times
    1 / h: 5.8e-6 of its size at 1024 nodes where 64 nodes give 1e-6.  Measured with one particle per node: the spread costs 3.6-5.5
    gathers, ``observe`` forward and backward 1.1-1.7 ms at 256^2 x 64 and 1.8-3.0 ms at 1024^2 x 8, 2.6-4.3x less than ``fields()`` with
    torch bilinear reads and autograd, whose scatter is atomic; particles clustered in 1 % of the cells spread 8-10x slower (the node
    launch's slot loops diverge).  Not built: the adjoint of ``advect`` (particle positions coupled back into the flow's adjoint),
    observing a velocity pair given as (u, v), a cotangent for the mean flow, sorting the positions themselves for gather locality."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * math.pi, Ly=2 * math.pi, drag=0.0, kappa=None, scalar_gradient=(0.0, 0.0),
                 buoyancy=(0.0, 0.0), hyperviscosity=None, hypofriction=None, beta=0.0):
        self.nx, self.ny = _pow2_axis('nx', nx), _pow2_axis('ny', ny)
        self.dt, self.rho = _real('dt', dt, '> 0'), _real('rho', rho, '> 0')
        self.nu = _real('nu', nu, '>= 0')
        self.Lx, self.Ly = _real('Lx', Lx, '> 0'), _real('Ly', Ly, '> 0')
        self.drag = _real('drag', drag, '>= 0')
        self.kappa = None if kappa is None else _real('kappa', kappa, '>= 0')
        self.scalar_gradient = _pair('scalar_gradient', scalar_gradient, '(Gx, Gy)')
        self.buoyancy = _pair('buoyancy', buoyancy, '(bx, by)')
        if self.buoyancy != (0.0, 0.0) and self.kappa is None:
            raise ValueError("buoyancy = %r needs a solver built with kappa (the diffusivity of the scalar that is buoyant)" % (self.buoyancy,))
        self.hyperviscosity = self._power_term('hyperviscosity', hyperviscosity, (0.0, 2))
        self.hypofriction = self._power_term('hypofriction', hypofriction, (0.0, 1))
        self.beta = _real('beta', beta, kind='hold real numbers')
        self.my1 = ops.spec_ns_kept_y(self.ny)
        self._lin = self._linear_table() if self._linear() else None      # (Re, Im)(lambda dt / 2), float32 numpy [my1, nx, 2]
        self._dev = collections.defaultdict(dict)                           # device copies of the host tables, by table ('lin', 'rate', 'stoch') and device
        self.ghat = None                       # the force's vorticity-equation spectrum g^, float32 [Bg, my1, nx, 2] (set_forcing)
        self.stoch_amp = None                  # the stochastic force's amplitude table a, float32 numpy [my1, nx] (set_stochastic_forcing)
        self.stoch_seed = 0
        self.last_simulate_used_graph = False

    def _on_device(self, key, dev, make):
        """Table ``key`` on device dev, from the host array make() when first needed there."""
        if dev not in self._dev[key]:
            self._dev[key][dev] = torch.from_numpy(np.ascontiguousarray(make())).to(dev)
        return self._dev[key][dev]

    @property
    def _lin_dev(self):                        # the linear table's device copies, by device (empty on a solver without the linear form)
        return self._dev['lin']

    def _work(self, query, B, dev, have=None):
        """A workspace of the size ``query`` (one of ops.spec_ns_*workspace) gives for B of this solver's grids, on dev: ``have`` where that
        is large enough, else a fresh one."""
        need = query(B, self.nx, self.ny)
        return have if have is not None and have.numel() >= need else torch.empty(need, dtype=torch.uint8, device=dev)

    def _at_rest(self, spectrum, work=None):
        """The state at rest around a spectrum [B, my1, nx, 2]: what ``fields`` and ``vorticity`` need to read it as a field."""
        B, dev = spectrum.shape[0], spectrum.device
        return PeriodicState(spectrum, torch.zeros((B, 2), dtype=torch.float32, device=dev),
                             self._work(ops.spec_ns_workspace, B, dev) if work is None else work)

    @staticmethod
    def _power_term(name, term, own, number=lambda name, c: _real(name, c, '>= 0')):
        """(coefficient, exponent) of ``hyperviscosity`` / ``hypofriction``; None: ``own``.  number(name, c) checks the coefficient: a real
        >= 0 at construction, also a 0-dim tensor in ``operator_table``."""
        coef, power, lo, hi = ('nu_h', 'p', 2, 8) if name == 'hyperviscosity' else ('mu', 'q', 1, 4)
        if term is None:
            return own
        try:
            c, n = term
        except (TypeError, ValueError):
            raise TypeError("%s must be None or (%s, %s), got %r" % (name, coef, power, term))
        c, n = number('%s of %s' % (coef, name), c), _int('%s of %s' % (power, name), n)
        if not lo <= n <= hi:
            raise ValueError("%s of %s = %d must be in [%d, %d]" % (power, name, n, lo, hi))
        return c, n

    def _field(self, name, a):
        if isinstance(a, np.ndarray):
            if a.dtype != np.float32:
                raise TypeError("%s: float32 fields expected, got %s" % (name, a.dtype))
            a = torch.from_numpy(np.ascontiguousarray(a))
        elif not isinstance(a, torch.Tensor):
            raise TypeError("%s: a torch tensor or numpy array expected, got %s" % (name, type(a).__name__))
        if a.dtype != torch.float32:
            raise TypeError("%s: float32 fields expected, got %s" % (name, a.dtype))
        if a.dim() == 2:
            a = a.unsqueeze(0)
        if a.dim() != 3 or tuple(a.shape[1:]) != (self.nx, self.ny) or a.shape[0] < 1:
            raise ValueError("%s: shape [B, %d, %d] expected, got %s" % (name, self.nx, self.ny, tuple(a.shape)))
        return a

    def _state(self, state):
        if not isinstance(state, PeriodicState):
            raise TypeError("a PeriodicState (from init) expected, got %s" % type(state).__name__)
        if tuple(state.what.shape[1:]) != (self.my1, self.nx, 2):
            raise ValueError("state of another grid: what is %s, this solver's is [B, %d, %d, 2]" % (tuple(state.what.shape), self.my1, self.nx))
        if state.that is not None:
            if tuple(state.that.shape) != tuple(state.what.shape):
                raise ValueError("the state's scalar spectrum is %s, its vorticity spectrum %s" % (tuple(state.that.shape), tuple(state.what.shape)))
            if self.kappa is None:
                raise ValueError("the state carries a scalar, this solver has no kappa")
        return state

    def init(self, u, v, theta=None):
        """State of velocity (u, v) ([B, nx, ny] or [nx, ny], float32): see the class note on the projection.  With ``theta`` (same shape) the
        state also carries the passive scalar: its band-limited part, the grid mean included (the solver needs ``kappa``)."""
        u, v = self._field('u', u), self._field('v', v)
        if u.shape != v.shape:
            raise ValueError("u and v must share their shape")
        if theta is not None:
            if self.kappa is None:
                raise ValueError("init(theta=...) needs a solver built with kappa (the scalar's diffusivity)")
            theta = self._field('theta', theta)
            if theta.shape != u.shape:
                raise ValueError("theta must have the shape of u and v")
        dev = u.device if u.is_cuda else (v.device if v.is_cuda else _device())
        u, v = u.to(dev).contiguous(), v.to(dev).contiguous()
        B = u.shape[0]
        what = torch.empty((B, self.my1, self.nx, 2), dtype=torch.float32, device=u.device)
        mean = torch.empty((B, 2), dtype=torch.float32, device=u.device)
        work = self._work(ops.spec_ns_workspace if theta is None else ops.spec_ns_scalar_workspace, B, u.device)
        ops.spec_ns_init(u, v, what, mean, work, self.Lx, self.Ly)
        that = None if theta is None else ops.spec_ns_scalar_init(theta.to(dev).contiguous(), torch.empty_like(what), work)
        state = PeriodicState(what, mean, work, that)
        if self.stoch_amp is not None:
            self._noise_of(state)
        if self._linear():
            self._linear_of(state)
        return state

    # ---- forcing
    def set_forcing(self, fx, fy=None):
        """Body force (fx, fy), constant in time: float32 [nx, ny] or [1, nx, ny] (shared by every grid of a batch) or [B, nx, ny] (one per
        grid; the states stepped afterwards must have that batch).  Only its solenoidal, zero-mean, band-limited part acts
        (``forcing_fields``); its spectrum g^ = M (i kx fy^ - i ky fx^) is built on the device and kept as ``self.ghat``.
        ``set_forcing(None)`` removes the force."""
        if fx is None:
            if fy is not None:
                raise ValueError("set_forcing: fx is None but fy is not")
            self.ghat = None
            return self
        fx, fy = self._field('fx', fx), self._field('fy', fy)
        if fx.shape != fy.shape:
            raise ValueError("fx and fy must share their shape")
        self.ghat = self.init(fx, fy).what          # the force is to g^ what the velocity is to w^
        return self

    def kolmogorov_forcing(self, k=4, amplitude=1.0):
        """f = (amplitude sin(2 pi k y / Ly), 0), shared by the batch; k an integer wavenumber inside the kept band (1 <= k, 3 k < ny)."""
        k = _int('k', k)
        if not (1 <= k and 3 * k < self.ny):
            raise ValueError("k = %d is outside the kept band 1 <= k, 3 k < ny = %d" % (k, self.ny))
        y = np.arange(self.ny) / float(self.ny)
        fx = np.broadcast_to(_real('amplitude', amplitude) * np.sin(2 * np.pi * k * y), (self.nx, self.ny)).astype(np.float32)
        return self.set_forcing(fx, np.zeros_like(fx))

    def forcing_fields(self):
        """(f_sx, f_sy) float32 [Bg, nx, ny]: the part of the force that acts (None without a force)."""
        if self.ghat is None:
            return None
        rest = self._at_rest(self.ghat)
        return ops.spec_ns_fields(rest.what, rest.mean, rest.work, self.ny, self.Lx, self.Ly, self.rho)[:2]

    def _forced(self):
        return self.ghat is not None or self.drag > 0

    # ---- stochastic forcing
    def _shell_table(self):
        """(S, shell [my1, nx] int, |k|^2 [my1, nx], kept [my1, nx] bool, wt [my1, 1], kx [1, nx]) of the stored modes, float64 on the host: the shell predicate
        floor(|k| / dk + 1/2) of ``shells()``, the step's 2/3 mask without (0, 0), and the weights 1 on j = 0, 2 on j > 0."""
        S, dk = ops.spec_ns_shells(self.nx, self.ny, self.Lx, self.Ly)
        mx = np.fft.fftfreq(self.nx) * self.nx
        j = np.arange(self.my1, dtype=np.float64)
        kx, ky = (2 * np.pi / self.Lx * mx)[None, :], (2 * np.pi / self.Ly * j)[:, None]
        k2 = kx * kx + ky * ky
        shell = np.floor(np.sqrt(k2) / dk + 0.5).astype(np.int64)
        kept = (3 * np.abs(mx)[None, :] < self.nx) & (k2 > 0)
        wt = np.where(j == 0, 1.0, 2.0)[:, None]
        return S, shell, k2, kept, wt, kx

    def shell_mode_counts(self):
        """float64 numpy [S]: N_s, the number of modes of the full spectrum in every shell that the step keeps (a stored mode with j > 0
        stands for itself and its conjugate)."""
        S, shell, k2, kept, wt, kx = self._shell_table()
        return np.bincount(shell[kept], weights=np.broadcast_to(wt, shell.shape)[kept], minlength=S)[:S]

    def set_stochastic_forcing(self, rate_by_shell, seed=0):
        """Gaussian white-in-time forcing with the mean energy injection rate ``rate_by_shell`` (float64 [S] over ``shells()``, each >= 0): a shell's
        rate eps_s is spread over its kept modes with equal energy per mode, a_k = |k| nx ny sqrt(2 eps_s / N_s), N_s = ``shell_mode_counts()``.
        The table is built on the host in float64 with the shell predicate floor(|k| / dk + 1/2) of ``shells()`` and kept as float32
        (``self.stoch_amp`` [my1, nx], shared by every grid of a batch).  ``seed``: an int in [0, 2^64), the generator's key; states stepped with
        the same seed, ``clock`` and ``noise_ids`` get the same noise.  A non-zero rate in a shell without a kept mode raises ValueError.
        ``set_stochastic_forcing(None)`` removes the forcing."""
        if rate_by_shell is None:
            self.stoch_amp, self.stoch_seed = None, 0
            self._dev.pop('stoch', None)
            return self
        seed = _seed(seed)
        S, shell, k2, kept, wt, kx = self._shell_table()
        try:
            rate = np.array(rate_by_shell, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError("rate_by_shell must be %d real numbers, got %r" % (S, rate_by_shell))
        if rate.shape != (S,):
            raise ValueError("rate_by_shell must have one entry per shell, [%d]; got %s" % (S, rate.shape))
        if not np.all(np.isfinite(rate)) or np.any(rate < 0):
            raise ValueError("rate_by_shell must be finite and >= 0")
        count = self.shell_mode_counts()
        empty = np.nonzero((rate > 0) & (count == 0))[0]
        if empty.size:
            raise ValueError("rate_by_shell is non-zero in shell %d, which holds no kept mode" % empty[0])
        per_mode = np.where(count > 0, 2.0 * rate / np.maximum(count, 1.0), 0.0)            # 2 eps_s / N_s
        inside = kept & (shell < S)
        amp = np.where(inside, np.sqrt(k2) * (self.nx * self.ny) * np.sqrt(per_mode[np.minimum(shell, S - 1)]), 0.0)
        self.stoch_amp, self.stoch_seed = np.ascontiguousarray(amp, dtype=np.float32), seed
        self._dev.pop('stoch', None)
        return self

    def ring_forcing(self, rate, k_lo, k_hi, seed=0):
        """``set_stochastic_forcing`` on the ring k_lo <= k_s <= k_hi of shell centres (``shells()``): the total mean injection ``rate`` > 0 is
        shared by those shells in proportion to their mode counts, so every forced mode gets the same energy input."""
        rate = _real('rate', rate, '> 0')
        k_lo, k_hi = _real('k_lo', k_lo, '>= 0'), _real('k_hi', k_hi, '>= 0')
        k = self.shells()[0]
        count = np.where((k >= k_lo) & (k <= k_hi), self.shell_mode_counts(), 0.0)
        if count.sum() == 0:
            raise ValueError("no kept mode lies in a shell with %r <= k_s <= %r" % (k_lo, k_hi))
        return self.set_stochastic_forcing(rate * count / count.sum(), seed)

    def stochastic_injection(self):
        """float64 numpy [S]: the exact mean energy injection rate of the stochastic force per shell, 1/2 sum wt a_k^2 / (|k|^2 (nx ny)^2) over the
        shell's stored kept modes, recomputed from the float32 table (zeros without the force).  Defined by the HOST's binning, the float64
        predicate floor(|k| / dk + 1/2) in NumPy: on a box where a mode sits within a rounding of a shell boundary the device's ``spectrum`` could
        bin it one shell over (with Lx = Ly = 2 pi it cannot: the square root of an integer is never s + 1/2)."""
        S, shell, k2, kept, wt, kx = self._shell_table()
        if self.stoch_amp is None:
            return np.zeros(S)
        a = self.stoch_amp.astype(np.float64)
        n2 = float(self.nx * self.ny) ** 2
        e = np.where(kept, 0.5 * wt * a * a / (np.where(kept, k2, 1.0) * n2), 0.0)
        return np.bincount(np.minimum(shell, S - 1)[kept], weights=e[kept], minlength=S)[:S]

    def _noise_of(self, state):
        """(amp, clock, noise_ids) on the state's device for a stochastic step; makes the state's clock (0) and ids (arange(B)) on first use --
        ``init`` does when the force is already set, so nothing is allocated inside a capture."""
        dev = state.what.device
        if state.clock is None:
            state.clock = torch.zeros(1, dtype=torch.int64, device=dev)
        if state.noise_ids is None:
            state.noise_ids = torch.arange(state.batch, dtype=torch.int32, device=dev)
        return self._on_device('stoch', dev, lambda: self.stoch_amp), state.clock, state.noise_ids

    # ---- linear operator
    def _linear(self):
        """Hyperviscosity, hypofriction or beta is active: the step takes the general linear form."""
        return self.hyperviscosity[0] > 0 or self.hypofriction[0] > 0 or self.beta != 0.0

    def linear_operator(self):
        """complex128 numpy [my1, nx], the layout of one grid of ``what``: lambda_k of the class note on the kept modes, 0 elsewhere and at (0, 0).
        Built on the host in float64; without the new terms it is -(nu |k|^2 + drag)."""
        S, shell, k2, kept, wt, kx = self._shell_table()
        k2 = np.where(kept, k2, 1.0)
        (nu_h, p), (mu, q) = self.hyperviscosity, self.hypofriction
        with np.errstate(over='ignore', invalid='ignore'):
            damp = self.nu * k2 + self.drag
            if nu_h > 0:
                damp = damp + nu_h * k2 ** p
            if mu > 0:
                damp = damp + mu * k2 ** (-q)
            lam = -damp + 1j * (self.beta * kx / k2)
        return np.where(kept, lam, 0.0)

    def _linear_table(self):
        """float32 numpy [my1, nx, 2] = (Re, Im)(lambda dt / 2), what the step reads; the angle is taken into [-pi, pi] in float64 first, which
        exp(lambda dt / 2) and exp(lambda dt) do not see and which keeps its float32 rounding small where beta dt / k is large."""
        with np.errstate(over='ignore', invalid='ignore'):
            half = self.linear_operator() * (0.5 * self.dt)
            table = np.stack([half.real, np.remainder(half.imag + np.pi, 2 * np.pi) - np.pi], axis=-1).astype(np.float32)
        if not np.all(np.isfinite(table)):
            raise ValueError("hyperviscosity = %r, hypofriction = %r, beta = %r: lambda dt / 2 is not finite in float32 on some kept mode"
                             % (self.hyperviscosity, self.hypofriction, self.beta))
        return np.ascontiguousarray(table)

    def _linear_of(self, state):
        """The table on the state's device (``init`` makes it, so nothing is allocated inside a capture)."""
        return self._on_device('lin', state.what.device, lambda: self._lin)

    def linear_spectrum(self, state):
        """LinearRates(k, energy, enstrophy), float64 [B, S] device tensors over ``shells()``: the rates at which the linear term changes the
        energy and the enstrophy of every shell, D_E(s) = sum wt Re(lambda_k) |w^_k|^2 / |k|^2 / (nx ny)^2 and D_Z(s) the same without 1 / |k|^2
        (weights and order of summation those of ``spectrum``), so that dE/dt|linear = sum_s D_E and dZ/dt|linear = sum_s D_Z.  beta contributes
        to neither (Im(lambda) only rotates a mode).  Works on any solver: without the new terms it is -2 nu Z(s) - 2 drag E(s) to rounding.
        Re(lambda) is taken from ``linear_operator()`` when first needed on a device.  Only reads the state."""
        self._state(state)
        rate = self._on_device('rate', state.what.device, lambda: self.linear_operator().real)
        out = ops.spec_ns_linear_spectrum(state.what, rate, self.ny, self.Lx, self.Ly)
        return LinearRates(self.shells()[0], out[:, 0], out[:, 1])

    def _force_of(self, state):
        """The force spectrum for this state (None without one); refuses a per-grid force of another batch or device before any launch."""
        g = self.ghat
        if g is not None:
            if g.shape[0] not in (1, state.batch):
                raise ValueError("the force is per grid for a batch of %d, the state has %d grids" % (g.shape[0], state.batch))
            if g.device != state.what.device:
                raise ValueError("the force is on %s, the state on %s" % (g.device, state.what.device))
        return g

    def _buoyant(self, state):
        """The scalar of this state acts on its flow: it has one and b != 0."""
        return state.that is not None and self.buoyancy != (0.0, 0.0)

    def _step_inputs(self, state, force=False, lin=None):
        """(ghat, lin, noise) of the step this solver takes on this state, and of the tangent step that rides on it.  force: False, the
        solver's own (``set_forcing``); else the spectrum g^ that takes its place (None: no force), as ``evolve`` passes its ``forcing``.
        lin: None, the solver's own table where it has one; else the table that takes its place, as ``evolve`` passes its ``operator``: the
        step is then the linear one on any solver.  noise: (amp, seed, clock, ids) of a stochastic solver, else None."""
        ghat = self._force_of(state) if force is False else force
        if lin is None and self._linear():
            lin = self._linear_of(state)
        noise = None
        if self.stoch_amp is not None:
            amp, clock, ids = self._noise_of(state)
            noise = (amp, self.stoch_seed, clock, ids)
        return ghat, lin, noise

    def _launch_steps(self, state, nsteps, force=False, lin=None):
        """The step this solver takes on this state, with the inputs of ``_step_inputs``; ops.spec_ns_advance_ picks the entry."""
        ghat, lin, noise = self._step_inputs(state, force, lin)
        ops.spec_ns_advance_(state.what, state.that, state.mean, ghat, state.work, self.ny, self.Lx, self.Ly, self.dt, self.nu, self.drag,
                             0.0 if self.kappa is None else self.kappa, self.scalar_gradient, self.buoyancy, lin, noise, nsteps)

    def step(self, state, nsteps=1):
        """nsteps time steps in place (no allocation, no host synchronisation)."""
        self._state(state)
        nsteps = _count('nsteps', nsteps, 0)
        self._launch_steps(state, nsteps)
        state.steps += nsteps
        return state

    # ---- forward mode
    def _tangent(self, who, spectra, state=None, members=False):
        """The checked tangent spectra of ``who``: (dwhat,) for a method of the flow alone, whose state must carry no scalar, (dwhat, dthat)
        for a ``_scalar`` method, whose solver needs ``kappa`` and whose state must carry one.  Each a contiguous float32 device tensor
        like ``state.what``, or with ``members`` K of them, [K, B, my1, nx, 2] (state None, the Gram matrix and the orthonormalisation: of
        any batch), dthat like dwhat.  Returns K (None without ``members``)."""
        scalar = len(spectra) == 2
        if scalar and self.kappa is None:
            raise ValueError("%s needs a solver built with kappa (the scalar's diffusivity); without a scalar use %s"
                             % (who, who.replace('_scalar', '')))
        if state is not None:
            self._state(state)
            if scalar and state.that is None:
                raise ValueError("%s: the state carries no scalar (build it with init(u, v, theta) on a solver with kappa); "
                                 "without one use %s" % (who, who.replace('_scalar', '')))
            if not scalar and state.that is not None:
                raise NotImplementedError("%s: the tangent of the scalar system is not built here: the state carries a scalar (passive or "
                                          "buoyant); use %s_scalar, or a state without one" % (who, who))
        want = (['K'] if members else []) + ['B' if state is None else state.batch, self.my1, self.nx, 2]
        for name, d in zip(('dwhat', 'dthat'), spectra):
            if not isinstance(d, torch.Tensor):
                raise TypeError("%s: %s must be a torch tensor, got %s" % (who, name, type(d).__name__))
            if d.dtype != torch.float32 or d.dim() != len(want) or tuple(d.shape[-3:]) != tuple(want[-3:]) or not d.is_cuda \
                    or not d.is_contiguous() or (state is not None and (d.shape[-4] != state.batch or d.device != state.what.device)):
                raise ValueError("%s: %s must be a contiguous float32 [%s] tensor on the %s, got %s %s on %s"
                                 % (who, name, ', '.join(map(str, want)), "device" if state is None else "state's device", d.dtype,
                                    tuple(d.shape), d.device))
        if scalar and (tuple(spectra[1].shape) != tuple(spectra[0].shape) or spectra[1].device != spectra[0].device):
            raise ValueError("%s: dwhat and dthat must share their shape and device, got %s on %s and %s on %s"
                             % (who, tuple(spectra[0].shape), spectra[0].device, tuple(spectra[1].shape), spectra[1].device))
        if not members:
            return None
        K = int(spectra[0].shape[0])
        if not 1 <= K <= ops.SPEC_NS_MAX_TANGENTS:
            raise ValueError("%s: K = %d tangents, must be in [1, %d]" % (who, K, ops.SPEC_NS_MAX_TANGENTS))
        return K

    def _launch_tangent(self, state, dwhat, dthat=None, K=None, nsteps=1, dghat=None, force=False):
        """``_launch_steps`` with a perturbation riding along, the inputs those of ``_step_inputs``, so the base is that step.  The one place
        that picks a tangent step's C entry: dthat None, the flow's tangent, else the pair's on a state with a scalar; K None, one tangent
        (which alone takes a source perturbation dghat), else K members [K, B, my1, nx, 2].  Grows ``state.work`` to that entry's workspace."""
        ghat, lin, noise = self._step_inputs(state, force)
        scalar, single = dthat is not None, K is None
        query, step = _TANGENT_STEPS[scalar, single]
        state.work = self._work(query if single else lambda B, nx, ny: query(B, K, nx, ny), state.batch, state.what.device, have=state.work)
        step(*((state.what, state.that, dwhat, dthat) if scalar else (state.what, dwhat)), state.mean, *((ghat, dghat) if single else (ghat,)),
             state.work, self.ny, self.Lx, self.Ly, self.dt, self.nu, self.drag,
             *((self.kappa, self.scalar_gradient, self.buoyancy) if scalar else ()), lin, noise, nsteps)

    def _dforcing(self, who, dforcing, state):
        """dg^ of the source perturbation ``dforcing`` ([B or 1, nx, ny] or [nx, ny]; None passes) for this state."""
        if dforcing is None:
            return None
        g = self._field('dforcing', dforcing.detach() if isinstance(dforcing, torch.Tensor) else dforcing)
        return self._source_spectrum(g.to(state.what.device), state)

    def step_tangent(self, state, dwhat, nsteps=1, dforcing=None):
        """``step(state, nsteps)`` -- bitwise, ``state.steps`` and ``state.clock`` included -- with the tangent spectrum ``dwhat`` (float32
        [B, my1, nx, 2], the layout of ``state.what``) advanced in place by the Jacobian of those steps and returned: the perturbation is
        carried along with the flow, each RK stage linearised about that stage's own state (the class note, "Forward mode").  Build ``dwhat``
        with ``init_vorticity(dw).what`` (or ``init(du, dv).what`` for a velocity perturbation) and read it with ``vorticity`` / ``fields`` of
        ``_at_rest(dwhat)``.  ``dforcing``: a perturbation of the vorticity source, float32 [B, nx, ny] or [1, nx, ny] (shared), constant over
        the call; its band-limited, zero-mean part acts.  Grows ``state.work`` to the tangent workspace on first use (take one step outside
        before capturing one in a graph); otherwise no allocation without ``dforcing`` and no host synchronisation.  A state that carries a
        scalar is refused: NotImplementedError."""
        self._tangent('step_tangent', (dwhat,), state)
        nsteps = _count('nsteps', nsteps, 0)
        self._launch_tangent(state, dwhat, None, None, nsteps, self._dforcing('step_tangent', dforcing, state))
        state.steps += nsteps
        return dwhat

    def _evolve_tangent(self, who, velocity, fields, dfields, nsteps, mean, forcing, dforcing, clock, noise_ids):
        """The four ``evolve*_tangent*``: the states of ``fields`` and of their perturbations ``dfields`` -- (w,) or (u0, v0), then theta for
        a ``_scalar`` method --, the tangent steps, and both read back in that order, the perturbation as a state at rest that carries
        dthat where there is one."""
        scalar = len(fields) > (2 if velocity else 1)
        if scalar and self.kappa is None:
            raise ValueError("%s needs a solver built with kappa (the scalar's diffusivity); without a scalar use %s"
                             % (who, who.replace('_scalar', '')))
        det = lambda a: a.detach() if isinstance(a, torch.Tensor) else a
        squeeze = isinstance(fields[0], (torch.Tensor, np.ndarray)) and fields[0].ndim == 2
        if velocity:
            state, dstate = self.init(*map(det, fields)), self.init(*map(det, dfields))
        else:
            def make(f, mean=None):
                st = self.init_vorticity(det(f[0]), mean)
                return self._with_scalar(who, st, f[1]) if scalar else st
            state, dstate = make(fields, mean), make(dfields)
        nsteps = _count('nsteps', nsteps, 1)
        if state.what.shape != dstate.what.shape:
            raise ValueError("%s: the fields and their perturbations must share their shape" % who)
        ghat = self._force_of(state) if forcing is None else self._source_spectrum(self._field('forcing', det(forcing)).to(state.what.device), state)
        if self.stoch_amp is not None:
            state.clock, state.noise_ids = self._noise_args(clock, noise_ids, state)
        self._launch_tangent(state, dstate.what, dstate.that, None, nsteps, self._dforcing(who, dforcing, state), ghat)
        state.steps += nsteps
        rest = self._at_rest(dstate.what, state.work)
        rest.that = dstate.that
        read = (lambda s: tuple(self.fields(s)[:2])) if velocity else (lambda s: (self.vorticity(s),))
        out = tuple(o for s in (state, rest) for o in read(s) + ((self.scalar(s),) if scalar else ()))
        return tuple(o[0] for o in out) if squeeze else out

    def evolve_tangent(self, w, dw, nsteps=1, mean=None, forcing=None, dforcing=None, clock=0, noise_ids=None):
        """(w_out, dw_out): the vorticity field after ``nsteps`` steps from w, bitwise ``evolve``'s forward, and the perturbation dw carried
        along with it, dw_out = J dw (+ the response to ``dforcing``), J the Jacobian of those steps -- the forward-mode twin of ``evolve``,
        whose backward gives J^T r: sum(dw_out * r) = sum(w.grad * dw) + sum(forcing.grad * dforcing) to float32 rounding.  w, dw: float32
        [B, nx, ny] or [nx, ny]; ``mean``, ``forcing`` (None: the force of ``set_forcing``, a constant), ``clock`` and ``noise_ids`` as in
        ``evolve``; ``dforcing``: the perturbation of the source, [B or 1, nx, ny].  The noise of a stochastic solver is a constant of the
        call: the base takes the kicks, the perturbation none.  NOT an autograd node: the inputs are detached and nothing is recorded.
        Nothing is stored per step.  No ``theta`` and no ``operator``."""
        return self._evolve_tangent('evolve_tangent', False, (w,), (dw,), nsteps, mean, forcing, dforcing, clock, noise_ids)

    def evolve_velocity_tangent(self, u0, v0, du0, dv0, nsteps=1, forcing=None, dforcing=None, clock=0, noise_ids=None):
        """``evolve_tangent`` from and to the velocity: (u, v, du, dv) after ``nsteps`` steps from (u0, v0) and the perturbation (du0, dv0):
        ``init`` of both (the perturbation's grid mean is dropped: the mean flow is a constant of the call), the tangent steps, ``fields`` of
        both.  (u, v) are bitwise ``evolve_velocity``'s forward.  NOT an autograd node: the inputs are detached."""
        return self._evolve_tangent('evolve_velocity_tangent', True, (u0, v0), (du0, dv0), nsteps, None, forcing, dforcing, clock, noise_ids)

    def _growth_rate(self, spectra, norm, step, nsteps, every):
        """The loop of ``lyapunov_exponent`` and ``lyapunov_exponent_scalar``: sum log(growth) / (nsteps dt) over segments of ``every``
        steps ``step(n)``, growth = sqrt(norm() after / before); at the start and after every segment each of ``spectra`` is rescaled, in
        their order, by the one float32 factor per grid that brings norm() to 1."""
        def rescale(e):                                  # to unit norm; the norm they then have, with the float32 factor as rounded
            f = torch.rsqrt(e).to(torch.float32)
            for d in spectra:
                d.mul_(f.reshape(-1, 1, 1, 1))
            return e * f.to(torch.float64) ** 2
        before = rescale(norm())
        total = torch.zeros_like(before)
        done = 0
        while done < nsteps:
            n = min(every, nsteps - done)
            step(n)
            after = norm()
            total += 0.5 * torch.log(after / before)
            before = rescale(after)
            done += n
        return total / (nsteps * self.dt)

    def lyapunov_exponent(self, state, dwhat, nsteps, renormalize_every):
        """The leading finite-time Lyapunov exponent of every grid in the energy norm, float64 [B] on the device: sum log(growth) / (nsteps dt)
        over ``nsteps`` steps of ``step_tangent`` (state and dwhat are advanced in place), growth = sqrt(E_after / E_before) of the
        perturbation's energy per segment of ``renormalize_every`` steps, after each of which (and at the start) dwhat is rescaled to unit
        energy: one torch multiply.  E is ``diagnostics(_at_rest(dwhat)).energy``, summed on the device in float64.  No host synchronisation:
        the caller's read of the result is the only one.  A grid whose perturbation has no energy gives nan."""
        self._tangent('lyapunov_exponent', (dwhat,), state)
        nsteps, every = _count('nsteps', nsteps, 1), _count('renormalize_every', renormalize_every, 1)
        return self._growth_rate((dwhat,), lambda: ops.spec_ns_diag(dwhat, None, self.ny, self.Lx, self.Ly)[:, 0],
                                 lambda n: self.step_tangent(state, dwhat, n), nsteps, every)

    # ---- forward mode of the system with a scalar
    def step_tangent_scalar(self, state, dwhat, dthat, nsteps=1, dforcing=None):
        """``step(state, nsteps)`` on a state that carries a scalar -- bitwise, ``state.steps`` and ``state.clock`` included -- with the tangent
        spectra ``dwhat`` and ``dthat`` (float32 [B, my1, nx, 2], the layout of ``state.what``) advanced in place by the Jacobian of those
        steps of the system (w^, theta^) and returned as (dwhat, dthat) (the class note, "Forward mode").  Build them with
        ``init_vorticity(dw).what`` and ``ops.spec_ns_scalar_init``; the mean of dtheta, the (0, 0) entry of dthat, is carried unchanged.
        ``dforcing`` as in ``step_tangent`` (the scalar has no source).  Grows ``state.work`` to the scalar tangent's workspace on first use
        (take one step outside before capturing one in a graph); otherwise no allocation without ``dforcing`` and no host synchronisation.
        ValueError on a state without a scalar."""
        self._tangent('step_tangent_scalar', (dwhat, dthat), state)
        nsteps = _count('nsteps', nsteps, 0)
        self._launch_tangent(state, dwhat, dthat, None, nsteps, self._dforcing('step_tangent_scalar', dforcing, state))
        state.steps += nsteps
        return dwhat, dthat

    def _with_scalar(self, who, state, theta):
        """``state`` (of init_vorticity) with the scalar theta, as ``evolve`` builds it."""
        if self.kappa is None:
            raise ValueError("%s needs a solver built with kappa (the scalar's diffusivity); without a scalar use %s"
                             % (who, who.replace('_scalar', '')))
        theta = self._field('theta', theta.detach() if isinstance(theta, torch.Tensor) else theta).to(state.what.device).contiguous()
        if theta.shape[0] != state.batch:
            raise ValueError("%s: the fields must share their shape" % who)
        state.that = ops.spec_ns_scalar_init(theta, torch.empty_like(state.what), state.work)
        return state

    def evolve_tangent_scalar(self, w, theta, dw, dtheta, nsteps=1, mean=None, forcing=None, dforcing=None, clock=0, noise_ids=None):
        """(w_out, theta_out, dw_out, dtheta_out): the fields after ``nsteps`` steps from (w, theta), bitwise the forward of
        ``evolve(w, nsteps, theta=theta, ...)``, and the perturbation (dw, dtheta) carried along with them by the Jacobian of those steps
        (+ the response to ``dforcing``) -- the forward-mode twin of ``evolve`` with a scalar, whose backward gives J^T r.  The arguments of
        ``evolve_tangent``; the solver needs ``kappa``.  NOT an autograd node: the inputs are detached and nothing is recorded."""
        return self._evolve_tangent('evolve_tangent_scalar', False, (w, theta), (dw, dtheta), nsteps, mean, forcing, dforcing, clock, noise_ids)

    def evolve_velocity_tangent_scalar(self, u0, v0, theta0, du0, dv0, dtheta0, nsteps=1, forcing=None, dforcing=None, clock=0, noise_ids=None):
        """``evolve_tangent_scalar`` from and to the velocity: (u, v, theta, du, dv, dtheta) after ``nsteps`` steps; (u, v, theta) are bitwise
        the forward of ``evolve_velocity(u0, v0, nsteps, theta0=theta0, ...)``.  The perturbation's grid-mean velocity is dropped.  NOT an
        autograd node: the inputs are detached."""
        return self._evolve_tangent('evolve_velocity_tangent_scalar', True, (u0, v0, theta0), (du0, dv0, dtheta0), nsteps, None, forcing, dforcing,
                                    clock, noise_ids)

    def lyapunov_exponent_scalar(self, state, dwhat, dthat, nsteps, renormalize_every, scalar_weight=1.0):
        """``lyapunov_exponent`` of the system with a scalar, float64 [B] on the device, in the norm E(dw) + scalar_weight 1/2 <dtheta'^2>
        (``scalar_weight`` > 0; the mean of dtheta does not enter): E is column 0 of ``ops.spec_ns_diag`` of dwhat, the variance column 0 of
        ``ops.spec_ns_scalar_diag`` of (dwhat, dthat), both summed on the device in float64, and both spectra are rescaled by the one factor
        after every ``renormalize_every`` steps of ``step_tangent_scalar`` (and at the start).  No host synchronisation."""
        self._tangent('lyapunov_exponent_scalar', (dwhat, dthat), state)
        nsteps, every = _count('nsteps', nsteps, 1), _count('renormalize_every', renormalize_every, 1)
        weight = _real('scalar_weight', scalar_weight, '> 0')
        norm = lambda: (ops.spec_ns_diag(dwhat, None, self.ny, self.Lx, self.Ly)[:, 0]
                        + weight * ops.spec_ns_scalar_diag(dwhat, dthat, self.ny, self.Lx, self.Ly, self.kappa)[:, 0])
        return self._growth_rate((dwhat, dthat), norm, lambda n: self.step_tangent_scalar(state, dwhat, dthat, n), nsteps, every)

    # ---- K tangents on one base
    def init_tangents(self, dw):
        """The spectra [K, B, my1, nx, 2] of K perturbation vorticity fields dw (float32 [K, B, nx, ny]): ``init_vorticity(dw[k]).what`` of
        every member, in one call on the K B fields (the band-limited part, the (0, 0) mode zeroed)."""
        dw = torch.as_tensor(dw)
        if dw.dim() != 4 or tuple(dw.shape[2:]) != (self.nx, self.ny):
            raise ValueError("dw: [K, B, %d, %d] expected, got %s" % (self.nx, self.ny, tuple(dw.shape)))
        K, B = int(dw.shape[0]), int(dw.shape[1])
        if not 1 <= K <= ops.SPEC_NS_MAX_TANGENTS:
            raise ValueError("init_tangents: K = %d tangents, must be in [1, %d]" % (K, ops.SPEC_NS_MAX_TANGENTS))
        return self.init_vorticity(dw.reshape(K * B, self.nx, self.ny)).what.reshape(K, B, self.my1, self.nx, 2)

    def step_tangents(self, state, dwhat, nsteps=1):
        """``step(state, nsteps)`` -- bitwise, ``state.steps`` and ``state.clock`` included -- with the K tangent spectra ``dwhat`` (float32
        [K, B, my1, nx, 2], ``init_tangents``) advanced in place and returned, every ``dwhat[k]`` bitwise as by ``step_tangent`` on a clone of
        the state (the class note, "Forward mode").  Grows ``state.work`` to the workspace of K tangents on first use (take one step outside
        before capturing one in a graph); otherwise no allocation and no host synchronisation.  A state that carries a scalar is refused:
        NotImplementedError."""
        K = self._tangent('step_tangents', (dwhat,), state, members=True)
        nsteps = _count('nsteps', nsteps, 0)
        self._launch_tangent(state, dwhat, None, K, nsteps)
        state.steps += nsteps
        return dwhat

    def tangent_gram(self, dwhat):
        """float64 [B, K, K] on the device: the Gram matrix of the K tangents of every grid in the energy inner product, 1/2 <du_k . du_l>;
        its diagonal is ``diagnostics(_at_rest(dwhat[k])).energy``.  Bitwise symmetric; two calls give the same bits."""
        self._tangent('tangent_gram', (dwhat,), members=True)
        return ops.spec_ns_tangent_gram(dwhat, self.ny, self.Lx, self.Ly)

    def orthonormalize_tangents(self, dwhat):
        """Orthonormalise the K tangents of every grid in place under the energy inner product, D = Q R with dwhat <- Q, and return
        log(diag R), float64 [B, K] on the device.  Cholesky QR done twice (the second pass restores the orthogonality that the first loses
        on nearly dependent vectors): the Gram matrix and the recombination d_k <- sum_{l <= k} (R^-1)[l, k] d_l touch the spectra and are
        HIP; the Cholesky factor and its triangular inverse are [B, K, K] float64 torch on the device, without error checks, so nothing
        synchronises.  The logs of the two passes add.  A grid whose vectors are dependent gives nan, as ``lyapunov_exponent`` does for a
        perturbation without energy."""
        K = self._tangent('orthonormalize_tangents', (dwhat,), members=True)
        return self._cholesky_qr_twice(K, dwhat.device, lambda: ops.spec_ns_tangent_gram(dwhat, self.ny, self.Lx, self.Ly),
                                       lambda rinv: ops.spec_ns_tangent_combine_(dwhat, rinv, self.ny))

    @staticmethod
    def _cholesky_qr_twice(K, device, gram_of, combine, pivot_floor=0.0):
        """The K x K algebra of ``orthonormalize_tangents`` and ``orthonormalize_tangents_scalar``: twice, the Gram matrix ``gram_of()``
        (float64 [B, K, K]) factored, ``combine(R^-1)`` applied to the vectors, the logs of diag R added.  nan where a pivot fails: it is not
        positive or (``pivot_floor`` > 0) R_kk^2 <= pivot_floor G_kk, a vector within rounding of the span of those before it."""
        eye = torch.eye(K, dtype=torch.float64, device=device)
        logs = None
        for _ in range(2):
            gram = gram_of()
            low, info = torch.linalg.cholesky_ex(gram, check_errors=False)                  # gram = low low^T: R = low^T
            rinv = torch.linalg.solve_triangular(low.transpose(-1, -2), eye.expand_as(gram), upper=True).contiguous()
            combine(rinv)
            diag = torch.diagonal(low, dim1=-2, dim2=-1)
            failed = (info != 0) | ~(diag > 0).all(dim=-1)                                  # a pivot that is not positive: dependent vectors
            if pivot_floor > 0:
                failed = failed | ~(diag * diag > pivot_floor * torch.diagonal(gram, dim1=-2, dim2=-1)).all(dim=-1)
            lg = torch.where(failed.unsqueeze(-1), torch.full_like(diag, float('nan')), torch.log(diag))
            logs = lg if logs is None else logs + lg
        return logs

    def _exponents(self, step, orthonormalize, nsteps, every):
        """The loop of ``lyapunov_spectrum`` and ``lyapunov_spectrum_scalar``: the sum of ``orthonormalize()``'s log(diag R) after every
        segment of ``every`` steps ``step(n)`` (the one at the start only orthonormalises) / (nsteps dt)."""
        total = torch.zeros_like(orthonormalize())
        done = 0
        while done < nsteps:
            n = min(every, nsteps - done)
            step(n)
            total += orthonormalize()
            done += n
        return total / (nsteps * self.dt)

    def lyapunov_spectrum(self, state, dwhat, nsteps, renormalize_every):
        """The first K finite-time Lyapunov exponents of every grid in the energy norm, float64 [B, K] on the device: the tangents are
        orthonormalised at the start and after every ``renormalize_every`` steps of ``step_tangents``, and the exponents are the sums of
        log(diag R) of those factorisations (the first one's excepted) / (nsteps dt).  State and dwhat are advanced in place; dwhat is left
        orthonormal: the backward Lyapunov vectors at the end of the run.  The exponents come in the order of the vectors, unsorted; they
        approach descending order as the run grows.  No host synchronisation.  A grid whose vectors become dependent gives nan."""
        self._tangent('lyapunov_spectrum', (dwhat,), state, members=True)
        nsteps, every = _count('nsteps', nsteps, 1), _count('renormalize_every', renormalize_every, 1)
        return self._exponents(lambda n: self.step_tangents(state, dwhat, n), lambda: self.orthonormalize_tangents(dwhat), nsteps, every)

    # ---- K tangent pairs on one base with a scalar
    def init_tangents_scalar(self, dw, dtheta):
        """(dwhat, dthat), [K, B, my1, nx, 2] each: the spectra of K perturbation pairs (dw, dtheta) (float32 [K, B, nx, ny] each).  dwhat is
        ``init_tangents(dw)``; dthat is ``ops.spec_ns_scalar_init`` on the K B fields: the band-limited part with the mean, the (0, 0) mode, kept."""
        if self.kappa is None:
            raise ValueError("init_tangents_scalar needs a solver built with kappa (the scalar's diffusivity); without a scalar use init_tangents")
        dwhat = self.init_tangents(dw)
        dtheta = torch.as_tensor(dtheta)
        if tuple(dtheta.shape) != tuple(torch.as_tensor(dw).shape):
            raise ValueError("dtheta: %s expected (the shape of dw), got %s" % (tuple(torch.as_tensor(dw).shape), tuple(dtheta.shape)))
        K, B = int(dwhat.shape[0]), int(dwhat.shape[1])
        theta = self._field('dtheta', dtheta.reshape(K * B, self.nx, self.ny)).to(dwhat.device).contiguous()
        flat = dwhat.reshape(K * B, self.my1, self.nx, 2)
        work = self._work(ops.spec_ns_workspace, K * B, dwhat.device)
        dthat = ops.spec_ns_scalar_init(theta, torch.empty_like(flat), work)
        return dwhat, dthat.reshape(K, B, self.my1, self.nx, 2)

    def step_tangents_scalar(self, state, dwhat, dthat, nsteps=1):
        """``step(state, nsteps)`` on a state that carries a scalar -- bitwise, ``state.steps`` and ``state.clock`` included -- with the K
        tangent pairs (``dwhat``, ``dthat``) (float32 [K, B, my1, nx, 2] each, ``init_tangents_scalar``) advanced in place and returned,
        every pair bitwise as by ``step_tangent_scalar`` on a clone of the state (the class note, "Forward mode").  Grows ``state.work`` to
        the workspace of K pairs on first use (take one step outside before capturing one in a graph); otherwise no allocation and no host
        synchronisation.  ValueError on a state without a scalar (use ``step_tangents``)."""
        K = self._tangent('step_tangents_scalar', (dwhat, dthat), state, members=True)
        nsteps = _count('nsteps', nsteps, 0)
        self._launch_tangent(state, dwhat, dthat, K, nsteps)
        state.steps += nsteps
        return dwhat, dthat

    def tangent_gram_scalar(self, dwhat, dthat, scalar_weight=1.0):
        """float64 [B, K, K] on the device: the Gram matrix of the K tangent pairs of every grid in the inner product of
        ``lyapunov_exponent_scalar``, 1/2 <du_k . du_l> + scalar_weight 1/2 <dtheta_k' dtheta_l'> (``scalar_weight`` > 0; the means of dtheta
        do not enter): ``tangent_gram(dwhat)`` + scalar_weight times the variance Gram matrix of dthat.  Bitwise symmetric and repeatable."""
        self._tangent('tangent_gram_scalar', (dwhat, dthat), members=True)
        weight = _real('scalar_weight', scalar_weight, '> 0')
        return ops.spec_ns_tangent_gram(dwhat, self.ny, self.Lx, self.Ly) + weight * ops.spec_ns_tangent_variance_gram(dthat, self.ny)

    def orthonormalize_tangents_scalar(self, dwhat, dthat, scalar_weight=1.0):
        """``orthonormalize_tangents`` of the K pairs under the inner product of ``tangent_gram_scalar``: (dwhat, dthat) <- Q in place, both
        spectra recombined with the one coefficient matrix (the means of dtheta combine with the rest: a tangent is linear), and
        log(diag R), float64 [B, K] on the device, returned.  The same Cholesky QR done twice, nan convention and absence of
        synchronisation.  The Gram matrix is a sum of two float64 matrices, so the pivot of an exactly dependent vector is rounding noise of
        either sign where the energy Gram alone cancels to zero: a pivot with R_kk^2 <= 1e-13 G_kk (450 float64 ulps; the nearly dependent
        sets a second pass can still repair sit near 1e-10) also counts as failed."""
        K = self._tangent('orthonormalize_tangents_scalar', (dwhat, dthat), members=True)
        weight = _real('scalar_weight', scalar_weight, '> 0')

        def combine(rinv):
            ops.spec_ns_tangent_combine_(dwhat, rinv, self.ny)
            ops.spec_ns_tangent_combine_(dthat, rinv, self.ny)
        return self._cholesky_qr_twice(K, dwhat.device, lambda: ops.spec_ns_tangent_gram(dwhat, self.ny, self.Lx, self.Ly)
                                       + weight * ops.spec_ns_tangent_variance_gram(dthat, self.ny), combine, pivot_floor=1e-13)

    def lyapunov_spectrum_scalar(self, state, dwhat, dthat, nsteps, renormalize_every, scalar_weight=1.0):
        """``lyapunov_spectrum`` of the system with a scalar, float64 [B, K] on the device, in the norm of ``lyapunov_exponent_scalar``: the
        pairs are orthonormalised (``orthonormalize_tangents_scalar``) at the start and after every ``renormalize_every`` steps of
        ``step_tangents_scalar``.  State and pairs are advanced in place; the pairs are left orthonormal.  ``kaplan_yorke_dimension`` applies
        to the result.  No host synchronisation."""
        self._tangent('lyapunov_spectrum_scalar', (dwhat, dthat), state, members=True)
        nsteps, every = _count('nsteps', nsteps, 1), _count('renormalize_every', renormalize_every, 1)
        _real('scalar_weight', scalar_weight, '> 0')
        return self._exponents(lambda n: self.step_tangents_scalar(state, dwhat, dthat, n),
                               lambda: self.orthonormalize_tangents_scalar(dwhat, dthat, scalar_weight), nsteps, every)

    # ---- reverse mode
    def _refuse_unsupported(self, who, scalar=False):
        """``advance*`` cover the forced, damped flow and, through the ``scalar`` entry points, its scalar and buoyancy; name the argument that
        puts a solver outside them and point at ``evolve`` / ``evolve_velocity``, which cover every solver."""
        if scalar and self.kappa is None:
            raise ValueError("%s needs a solver built with kappa (the scalar's diffusivity); without a scalar use %s"
                             % (who, who.replace('_scalar', '')))
        for name, on in (('buoyancy', self.buoyancy != (0.0, 0.0) and not scalar), ('kappa', self.kappa is not None and not scalar),
                         ('set_stochastic_forcing', self.stoch_amp is not None), ('hyperviscosity', self.hyperviscosity[0] > 0),
                         ('hypofriction', self.hypofriction[0] > 0), ('beta', self.beta != 0.0)):
            if on:
                raise NotImplementedError("%s: no reverse mode here for a solver with %s; use %s, which covers every solver"
                                          % (who, name, 'evolve_velocity' if 'velocity' in who else 'evolve'))

    def _grad_field(self, name, a):
        """A float32 device tensor [B, nx, ny] (or [nx, ny]) that autograd can follow: no copy from the host or another dtype."""
        if not isinstance(a, torch.Tensor):
            raise TypeError("%s: a torch tensor expected, got %s" % (name, type(a).__name__))
        if not a.is_cuda:
            raise TypeError("%s: a CUDA/HIP tensor expected (the HIP path has no CPU fallback)" % name)
        self._field(name, a)
        return a

    def _k2_table(self, dev, sign):
        """|k|^2 (sign 1) or 1 / |k|^2 (sign -1; 0 at (0, 0)) of the stored modes, float32 [my1, nx, 1] on dev, from float64 on the host."""
        def make():
            k2 = self._shell_table()[2]
            return (k2 if sign > 0 else np.where(k2 > 0, 1.0 / np.where(k2 > 0, k2, 1.0), 0.0)).astype(np.float32)[:, :, None]
        return self._on_device('k2' if sign > 0 else 'ik2', dev, make)

    def _source_spectrum(self, g, state):
        """g^ in the layout of what for the vorticity source g(x) [1 or B, nx, ny] of ``advance``: its band-limited, zero-mean part."""
        if g.shape[0] not in (1, state.batch) or g.device != state.what.device:
            raise ValueError("forcing: [1 or %d, %d, %d] on the state's device expected, got %s on %s"
                             % (state.batch, self.nx, self.ny, tuple(g.shape), g.device))
        return self.init_vorticity(g).what

    def init_vorticity(self, w, mean=None):
        """State of the vorticity field w ([B, nx, ny] or [nx, ny], float32) and the mean velocity ``mean`` ([B, 2] or a pair; None: at rest):
        keeps the band-limited part of w and zeroes its (0, 0) mode (a periodic velocity has a zero-mean vorticity)."""
        w = self._field('w', w)
        w = w.to(w.device if w.is_cuda else _device()).contiguous()
        B, dev = w.shape[0], w.device
        what = torch.empty((B, self.my1, self.nx, 2), dtype=torch.float32, device=dev)
        work = self._work(ops.spec_ns_scalar_workspace, B, dev)
        ops.spec_ns_scalar_init(w, what, work)
        what[:, 0, 0, :] = 0.0
        if mean is None:
            mean = torch.zeros((B, 2), dtype=torch.float32, device=dev)
        else:
            mean = torch.as_tensor(mean, dtype=torch.float32).to(dev).reshape(-1, 2).expand(B, 2).contiguous()
        return PeriodicState(what, mean, work)

    def vorticity(self, state, out=None):
        """w float32 [B, nx, ny] of the state (into ``out`` if given)."""
        self._state(state)
        work = self._work(ops.spec_ns_scalar_workspace, state.batch, state.what.device, have=state.work)
        return ops.spec_ns_scalar_field(state.what, work, self.ny, out)

    def _evolve(self, who, velocity, fields, nsteps, mean, forcing, clock, noise_ids, operator):
        """The six differentiable entry points: the checks, then one ``_AdvanceFn``.  ``fields``: (name, tensor) pairs, (w,) or (u0, v0), then
        theta iff the solver has ``kappa`` (its scalar is part of the state).  Returns the fields after ``nsteps`` steps in that order, a
        single one bare."""
        scalar = len(fields) > (2 if velocity else 1)
        if scalar != (self.kappa is not None):
            raise ValueError("%s: %s" % (who, "the solver has kappa: its scalar (theta) is part of the state and must be given" if not scalar
                                     else "a scalar (theta) needs a solver built with kappa (the scalar's diffusivity)"))
        nsteps = _count('nsteps', nsteps, 1)
        fields = [self._grad_field(name, f) for name, f in fields]
        if any(f.shape != fields[0].shape for f in fields[1:]):
            raise ValueError("%s: the fields must share their shape" % who if scalar else "u0 and v0 must share their shape")
        if forcing is not None:
            forcing = self._grad_field('forcing', forcing)
            if forcing.dim() == 2:
                forcing = forcing.unsqueeze(0)
        operator = self._operator_arg(who, operator, fields[0])
        out = _AdvanceFn.apply(_Run(self, nsteps, mean, velocity, scalar, (clock, noise_ids)), forcing, operator, *fields)
        return out[0] if len(out) == 1 else out

    def advance(self, w, nsteps=1, mean=None, forcing=None):
        """``evolve`` on the solvers it was written for, the steady-forced, damped flow: the vorticity field after ``nsteps`` steps from w,
        differentiable in w and ``forcing``, bitwise ``evolve``'s outputs and gradients.  Not for a solver with kappa or buoyancy
        (``advance_scalar`` / ``advance_velocity_scalar`` take and return the scalar) and not for a stochastic force, hyperviscosity,
        hypofriction or beta: NotImplementedError; ``evolve`` covers every solver.  No ``operator``, ``clock`` or ``noise_ids``."""
        self._refuse_unsupported('advance')
        return self._evolve('advance', False, (('w', w),), nsteps, mean, forcing, 0, None, None)

    def advance_velocity(self, u0, v0, nsteps=1, forcing=None):
        """``advance`` from and to the velocity: (u, v) after ``nsteps`` steps from (u0, v0), as ``evolve_velocity``.  The refusals of
        ``advance``; ``evolve_velocity`` covers every solver."""
        self._refuse_unsupported('advance_velocity')
        return self._evolve('advance_velocity', True, (('u0', u0), ('v0', v0)), nsteps, None, forcing, 0, None, None)

    def advance_scalar(self, w, theta, nsteps=1, mean=None, forcing=None):
        """``evolve`` with ``theta`` on a solver with ``kappa`` (and ``buoyancy``): (w, theta) after ``nsteps`` steps, differentiable in w,
        theta and ``forcing``.  ValueError on a solver without kappa; not for a stochastic force, hyperviscosity, hypofriction or beta:
        NotImplementedError (``evolve`` covers every solver)."""
        self._refuse_unsupported('advance_scalar', scalar=True)
        return self._evolve('advance_scalar', False, (('w', w), ('theta', theta)), nsteps, mean, forcing, 0, None, None)

    def advance_velocity_scalar(self, u0, v0, theta0, nsteps=1, forcing=None):
        """``advance_scalar`` from and to the velocity: (u, v, theta) after ``nsteps`` steps, as ``evolve_velocity``.  The refusals of
        ``advance_scalar``; ``evolve_velocity`` covers every solver."""
        self._refuse_unsupported('advance_velocity_scalar', scalar=True)
        return self._evolve('advance_velocity_scalar', True, (('u0', u0), ('v0', v0), ('theta0', theta0)), nsteps, None, forcing, 0, None, None)

    # ---- the linear operator as an argument of evolve
    def _operator_arg(self, who, operator, field):
        """The checked ``operator`` of ``evolve`` / ``evolve_velocity`` (None passes): a float32 tensor [my1, nx, 2] on the fields' device."""
        if operator is None:
            return None
        if not isinstance(operator, torch.Tensor):
            raise TypeError("%s: operator must be a torch tensor, got %s" % (who, type(operator).__name__))
        if operator.dtype != torch.float32:
            raise TypeError("%s: operator must be float32, got %s" % (who, operator.dtype))
        if tuple(operator.shape) != (self.my1, self.nx, 2):
            raise ValueError("%s: operator must be [%d, %d, 2] = (Re, Im)(lambda dt / 2) of the stored modes, got %s"
                             % (who, self.my1, self.nx, tuple(operator.shape)))
        if operator.device != field.device:
            raise ValueError("%s: operator is on %s, the fields on %s" % (who, operator.device, field.device))
        return operator

    def _operator_of(self, operator, state):
        """What the step reads of an ``operator``: its values, contiguous, on the state's device."""
        if operator.device != state.what.device:
            raise ValueError("operator is on %s, the state on %s" % (operator.device, state.what.device))
        return operator.detach().contiguous()

    def _operator_gradient(self, lbar):
        """The gradient in the table, float32 [my1, nx, 2], from the per-grid sums lbar [B, my1, nx, 2] of ops.spec_ns_step_operator_adjoint_
        (include/nns.h has the definition): the grids summed in a fixed order (one deterministic torch.sum), a stored mode with ky > 0 weighted
        2 / (nx ny) for itself and its mirror image, and the ky = 0 line, which stores both kx and -kx, made (T(kx) + conj(T(-kx))) / (2 nx ny):
        the part of the cotangent that a table with l(-k) = conj(l(k)) can feel, exactly symmetric in float32 (the sum commutes, the weights are
        powers of two)."""
        T = torch.sum(lbar, dim=0)
        n = float(self.nx * self.ny)
        G = T * (2.0 / n)
        mirror = T[0, (-torch.arange(self.nx, device=T.device)) % self.nx]
        G[0, :, 0] = (T[0, :, 0] + mirror[:, 0]) * (0.5 / n)
        G[0, :, 1] = (T[0, :, 1] - mirror[:, 1]) * (0.5 / n)
        return G

    def mode_table(self, device=None):
        """(kx, ky, k2, kept) of the stored modes in the layout of one grid of ``what`` and of ``operator``, [my1, nx] on ``device`` (None: the
        default device): the wavenumbers and |k|^2 as float64, and the bool mask of the modes the step keeps (the 2/3 band without (0, 0)).
        Row j holds ky = 2 pi j / Ly >= 0, column e the kx of numpy.fft.fftfreq; row 0 holds both kx and -kx.  With it an ``operator`` can be
        written as a function of k, e.g. a network of |k| for a learned eddy viscosity: Re = -nu(|k|) k2 dt / 2 on ``kept``, 0 elsewhere."""
        dev = _device(device)
        S, shell, k2, kept, wt, kx = self._shell_table()
        ky = 2 * np.pi / self.Ly * np.arange(self.my1, dtype=np.float64)[:, None]
        t = lambda a: torch.from_numpy(np.array(np.broadcast_to(a, k2.shape))).to(dev)            # a writable copy
        return t(kx), t(ky), t(k2), t(kept)

    def operator_table(self, nu=None, drag=None, hyperviscosity=None, hypofriction=None, beta=None, device=None):
        """The table ``evolve(..., operator=)`` takes, float32 [my1, nx, 2] = (Re, Im)(lambda_k dt / 2) on ``device`` (None: the default device),
        built from the class note's formula as a differentiable torch function of its parameters:
            lambda_k = -(nu |k|^2 + drag + nu_h |k|^2p + mu |k|^-2q) + i beta kx / |k|^2 on the kept modes, 0 elsewhere and at (0, 0).
        nu, drag, beta: Python numbers or 0-dim tensors that may require grad; ``hyperviscosity`` = (nu_h, p) and ``hypofriction`` = (mu, q) with
        nu_h, mu such and p, q Python ints (the powers |k|^2p, |k|^-2q are made on the host in float64 and are constants).  None: the solver's
        own value.  So ``evolve(w, n, operator=solver.operator_table(nu=nu_t))`` followed by backward() puts d loss / d nu in nu_t.grad, and
        likewise for drag, nu_h, mu and beta, with no kernel beyond the table's.  Computed in float64 on the device in the order of
        ``linear_operator`` / ``_linear_table`` (the angle taken into [-pi, pi] the same way) and cast to float32: with the solver's own
        numbers it is the solver's table.  Signs and finiteness are not checked (that would synchronise with the host)."""
        dev = _device(device)
        S, shell, k2, kept, wt, kx = self._shell_table()
        k2 = np.where(kept, k2, 1.0)
        f64 = lambda a: torch.from_numpy(np.array(np.broadcast_to(a, k2.shape), dtype=np.float64)).to(dev)      # a writable copy

        def number(name, x, own=None):
            if x is None:
                return own
            if isinstance(x, torch.Tensor):
                if x.dim() != 0:
                    raise ValueError("%s must be a number or a 0-dim tensor, got shape %s" % (name, tuple(x.shape)))
                return x.to(device=dev, dtype=torch.float64)
            return _real(name, x, kind='hold real numbers')

        nu, drag, beta = number('nu', nu, self.nu), number('drag', drag, self.drag), number('beta', beta, self.beta)
        nu_h, p = self._power_term('hyperviscosity', hyperviscosity, self.hyperviscosity, number)
        mu, q = self._power_term('hypofriction', hypofriction, self.hypofriction, number)
        on = lambda c: isinstance(c, torch.Tensor) or c > 0          # linear_operator's own test for a Python number
        k2d, keptd = f64(k2), torch.from_numpy(np.ascontiguousarray(kept)).to(dev)
        with np.errstate(over='ignore', invalid='ignore'):
            damp = nu * k2d + drag
            if on(nu_h):
                damp = damp + nu_h * f64(k2 ** p)
            if on(mu):
                damp = damp + mu * f64(k2 ** (-q))
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        re = torch.where(keptd, -damp + 0.0, zero) * (0.5 * self.dt)        # + 0.0: an undamped mode is +0, as the complex sum makes it there
        im = torch.where(keptd, (beta * f64(kx)) / k2d, zero) * (0.5 * self.dt)
        im = torch.remainder(im + np.pi, 2 * np.pi) - np.pi
        return torch.stack([re, im], dim=-1).to(torch.float32)

    def _noise_args(self, clock, noise_ids, state):
        """(clock, noise_ids) of ``evolve`` as a state's: clock an int >= 0 or an int64 device tensor [1], copied (the step advances the copy);
        noise_ids None (arange(B)) or B ints."""
        dev, B = state.what.device, state.batch
        if isinstance(clock, torch.Tensor):
            if clock.dtype != torch.int64 or tuple(clock.shape) != (1,) or clock.device != dev:
                raise ValueError("clock: an int or an int64 tensor [1] on the state's device expected, got %s %s on %s"
                                 % (clock.dtype, tuple(clock.shape), clock.device))
            clock = clock.clone()
        else:
            clock = torch.full((1,), _count('clock', clock, 0), dtype=torch.int64, device=dev)
        if noise_ids is None:
            ids = torch.arange(B, dtype=torch.int32, device=dev)
        else:
            ids = torch.as_tensor(noise_ids).to(device=dev, dtype=torch.int32).reshape(-1).contiguous().clone()
            if ids.numel() != B:
                raise ValueError("noise_ids: one id per grid, [%d], expected, got %d" % (B, ids.numel()))
        return clock, ids

    def evolve(self, w, nsteps=1, theta=None, mean=None, forcing=None, clock=0, noise_ids=None, operator=None):
        """The vorticity field after ``nsteps`` steps of ANY solver from the vorticity field w (float32 device tensor [B, nx, ny] or [nx, ny];
        with ``theta``, required iff the solver has ``kappa``: the pair (w, theta)), differentiable in w, theta and ``forcing``: one autograd
        node, so a closure, a learned forcing or an initial condition can be trained THROUGH the solver.  The forward takes the step ``step``
        takes -- linear (hyperviscosity, hypofriction, beta), stochastic, buoyant, scalar, forced or plain -- and is bitwise ``step`` on
        ``init_vorticity(w, mean)`` (``that`` from ``ops.spec_ns_scalar_init(theta)``), read by ``vorticity`` and ``scalar``; the backward is
        the adjoint of the Lawson RK4 step as HIP kernels (csrc/pspec_kernels.hip: ps_row_adj_kernel, ps_col_adj_kernel; derivation in
        DESIGN.md section 4.2), the scalar riding in the flow's launches, with the conjugate Lawson factors conj(E), conj(E^2) read from the
        forward's table on a solver with the general linear operator.  A stochastic step is differentiated as the deterministic step it
        contains: the kick is additive and independent of the state, and the saved start spectra carry it.
        ``forcing``: a vorticity source g(x), float32 device tensor [B or 1, nx, ny], constant over the call, differentiable too (for a shared
        one the per-grid gradients are summed, one deterministic torch.sum); None: the force of ``set_forcing``, a constant.  The scalar has
        no source.  ``mean``: the mean velocity ([B, 2] or a pair; None: at rest), a constant of the motion that is not differentiated.
        ``clock``: the index of the first step's noise, an int or an int64 device tensor [1] that is copied, never advanced: a rollout cut
        into chunks passes n0, n0 + nsteps, ... and reproduces the uncut noise; ``noise_ids`` as on ``PeriodicState`` (None: arange(B)).  Both
        are ignored without a stochastic force.  kappa, G, b, the mean flow, the amplitudes and the seed are constants and are not
        differentiated, and without ``operator`` nu, drag and the table are too.  Memory kept for the backward: the spectrum (with a scalar:
        both) at the start of every step, nsteps x B x my1 x nx x 8 (16) bytes, my1 = (ny - 1) // 3 + 1: a third of a field per step and
        grid; the stages inside a step are recomputed.
        ``operator``: None, or a float32 device tensor [my1, nx, 2] = (Re, Im)(lambda_k dt / 2) in the solver's table layout (``mode_table``
        names the modes) that takes the place of the solver's own linear operator in this call -- ``operator_table(nu=..., drag=...)`` builds
        one from physical parameters, a network of |k| a learned one.  The call then takes the LINEAR step with that table, on any solver, and
        is differentiable in it: the backward sums the table's cotangent in the adjoint's own launches (the class note).  The table must obey
        l(-k) = conj(l(k)) on the ky = 0 line, where both kx and -kx are stored, and should have Re <= 0; neither is checked.  The gradient
        returned obeys the symmetry, is zero off the kept modes and at (0, 0), and the gradients of the fields and of ``forcing`` are bitwise
        those of the call without the table's gradient."""
        fields = (('w', w),) if theta is None else (('w', w), ('theta', theta))
        return self._evolve('evolve', False, fields, nsteps, mean, forcing, clock, noise_ids, operator)

    def evolve_velocity(self, u0, v0, nsteps=1, theta0=None, forcing=None, clock=0, noise_ids=None, operator=None):
        """``evolve`` from and to the velocity: (u, v), or with ``theta0`` (required iff the solver has ``kappa``) (u, v, theta), after ``nsteps``
        steps: ``fields(step(init(u0, v0, theta0), nsteps))[:2]`` (and ``scalar`` of it) forward; backward through the velocity by
        K^T (ubar, vbar)^ = curl(ubar, vbar)^ / |k|^2, the step's adjoint, and init^T (lam) = (lam_y, -lam_x), built from the init / fields
        kernels and one |k|^-2, |k|^2 table multiply each.  The grid means (U0, V0) of (u0, v0) are constants of the motion and are not
        differentiated.  No pressure output.  ``forcing``, ``clock``, ``noise_ids`` and ``operator`` as in ``evolve``."""
        fields = (('u0', u0), ('v0', v0)) if theta0 is None else (('u0', u0), ('v0', v0), ('theta0', theta0))
        return self._evolve('evolve_velocity', True, fields, nsteps, None, forcing, clock, noise_ids, operator)

    # ---- second order: reverse mode through the tangent
    def second_order_forward(self, w, dw, nsteps=1, mean=None, forcing=None, dforcing=None, clock=0, noise_ids=None):
        """The forward half of a Hessian-vector product through ``nsteps`` steps: ``evolve_tangent`` taken in one-step calls with the
        spectra (w^, dw^) at the start of every step kept, nsteps x B x my1 x nx x 16 bytes.  Returns a ``SecondOrderRun`` whose ``.w`` is
        bitwise ``evolve``'s forward and ``.dw`` bitwise ``evolve_tangent``'s, and whose ``backward(lam, dlam)`` is the second-order adjoint
        (its note).  The arguments are ``evolve_tangent``'s.  Plain, forced, linear (hyperviscosity, hypofriction, beta, drag) and stochastic
        solvers; a solver with ``kappa`` is refused, NotImplementedError: the second-order adjoint of the scalar system is not built.  NOT an
        autograd node: the inputs are detached.  No ``operator`` and no velocity ends."""
        if self.kappa is not None:
            raise NotImplementedError("second_order_forward: the second-order adjoint of the scalar system is not built (this solver has kappa)")
        nsteps = _count('nsteps', nsteps, 1)
        det = lambda a: a.detach() if isinstance(a, torch.Tensor) else a
        squeeze = isinstance(w, (torch.Tensor, np.ndarray)) and w.ndim == 2
        state, dstate = self.init_vorticity(det(w), mean), self.init_vorticity(det(dw))
        if state.what.shape != dstate.what.shape:
            raise ValueError("second_order_forward: the field and its perturbation must share their shape")
        given = forcing is not None
        if given:
            forcing = self._field('forcing', det(forcing)).to(state.what.device)
            ghat = self._source_spectrum(forcing, state)
        else:
            ghat = self._force_of(state)
        dghat = self._dforcing('second_order_forward', dforcing, state)
        if self.stoch_amp is not None:
            state.clock, state.noise_ids = self._noise_args(clock, noise_ids, state)
        what0 = torch.empty((nsteps,) + tuple(state.what.shape), dtype=torch.float32, device=state.what.device)
        dwhat0 = torch.empty_like(what0)
        for k in range(nsteps):
            what0[k].copy_(state.what)
            dwhat0[k].copy_(dstate.what)
            self._launch_tangent(state, dstate.what, None, None, 1, dghat, ghat)
        out = self.vorticity(state), self.vorticity(self._at_rest(dstate.what, state.work))
        return SecondOrderRun(self, tuple(o[0] for o in out) if squeeze else out, what0, dwhat0, state.mean, ghat, dghat,
                              self._linear_of(state) if self._linear() else None, tuple(forcing.shape) if given else None, squeeze)

    def hessian_vector_product(self, loss, w, dw, nsteps=1, mean=None, forcing=None, dforcing=None, clock=0, noise_ids=None):
        """(loss, grad_w, grad_forcing, hvp_w, hvp_forcing) of l(w, forcing) = ``loss``(the vorticity field after ``nsteps`` steps from w): the
        value, the gradient and the exact Hessian-vector product H (dw, dforcing), in one tangent forward and one second-order backward where a
        finite difference of gradients takes two forward and two backward passes and loses the digits the gradients share.  ``loss`` maps the
        final field ([B, nx, ny], or [nx, ny] for such a w) to a scalar tensor by torch operations; lam = dl/dw_N is taken by autograd and
        dlam = (d^2 l / dw_N^2) dw_N by a second ``torch.autograd.grad`` of <lam, dw_N>, zero where lam carries no graph (a linear loss).  The
        Gauss-Newton product J^T (d^2 l) J d is the part that comes from dlam; the rest, sum lam . d^2 Phi[d, .], is what a first-order code
        cannot give.  The forcing entries are None without ``forcing``; for a shared one ([1, nx, ny]) they are summed over the batch.  H is
        symmetric: sum(a . H b) = sum(b . H a) to float32 rounding, jointly in (w, forcing).  The other arguments and the refusals are
        ``second_order_forward``'s."""
        run = self.second_order_forward(w, dw, nsteps, mean, forcing, dforcing, clock, noise_ids)
        with torch.enable_grad():
            w1 = run.w.detach().requires_grad_(True)
            value = loss(w1)
            if not (isinstance(value, torch.Tensor) and value.numel() == 1):
                raise TypeError("hessian_vector_product: loss must return a scalar tensor")
            lam, = torch.autograd.grad(value, w1, create_graph=True)
            dlam = None
            if lam.requires_grad:
                dlam, = torch.autograd.grad(torch.sum(lam * run.dw), w1, allow_unused=True)
        if dlam is None:
            dlam = torch.zeros_like(run.w)
        out = run.backward(lam.detach(), dlam.detach())
        return value.detach(), out.wbar, out.gbar, out.dwbar, out.dgbar

    def diagnostics(self, state):
        """Diagnostics(energy, enstrophy, power_in), each float64 [B], computed on the device from the state's spectrum:
        energy = 1/2 <|u - <u>|^2> (the total is energy + (U0^2 + V0^2) / 2), enstrophy = 1/2 <w^2>, power_in = <f_s . u> (exactly 0
        without a force), so that d energy / dt = power_in - 2 nu enstrophy - 2 drag energy; with the general linear operator of the class note
        d energy / dt = power_in + sum_s D_E(s), D_E of ``linear_spectrum``, which holds on every solver."""
        self._state(state)
        out = ops.spec_ns_diag(state.what, self._force_of(state), self.ny, self.Lx, self.Ly)
        return Diagnostics(out[:, 0], out[:, 1], out[:, 2])

    def _scalar_state(self, state):
        self._state(state)
        if state.that is None:
            raise ValueError("the state carries no scalar: build it with init(u, v, theta) on a solver with kappa")
        return state

    def scalar(self, state, out=None):
        """theta float32 [B, nx, ny] of the state (into ``out`` if given)."""
        self._scalar_state(state)
        return ops.spec_ns_scalar_field(state.that, state.work, self.ny, out)

    def scalar_diagnostics(self, state):
        """ScalarDiagnostics(variance, dissipation, flux_x, flux_y), each float64 [B], computed on the device from the state's spectra:
        variance = 1/2 <theta'^2> (theta' = theta - <theta>), dissipation = kappa <|grad theta|^2>, flux = <u theta'>, so that
        d variance / dt = -(Gx flux_x + Gy flux_y) - dissipation."""
        self._scalar_state(state)
        out = ops.spec_ns_scalar_diag(state.what, state.that, self.ny, self.Lx, self.Ly, self.kappa)
        return ScalarDiagnostics(out[:, 0], out[:, 1], out[:, 2], out[:, 3])

    # ---- by wavenumber
    def shells(self):
        """(k, dk): the shell centres k_s = s dk, a float64 numpy array [S], and the shell width dk = min(2 pi / Lx, 2 pi / Ly).  A stored
        mode belongs to shell floor(|k| / dk + 1/2); S - 1 is the shell of the kept band's corner and shell 0 is empty."""
        S, dk = ops.spec_ns_shells(self.nx, self.ny, self.Lx, self.Ly)
        return dk * np.arange(S, dtype=np.float64), dk

    def spectrum(self, state):
        """Spectrum(k, energy, enstrophy, injection, variance): k as ``shells()``; the others float64 [B, S] device tensors, per shell the
        sums that ``diagnostics`` (energy, enstrophy, power_in) and ``scalar_diagnostics`` (variance) take over the whole band.  injection is
        zeros without a force; variance is None for a state without a scalar.  Only reads the state."""
        self._state(state)
        out = ops.spec_ns_spectrum(state.what, state.that, self._force_of(state), self.ny, self.Lx, self.Ly)
        return Spectrum(self.shells()[0], out[:, 0], out[:, 1], out[:, 2], None if state.that is None else out[:, 3])

    def transfer(self, state):
        """Transfer(k, energy, enstrophy, variance), float64 [B, S] device tensors: the rate at which the nonlinear term moves energy,
        enstrophy and scalar variance INTO every shell, T_Z(s) = sum Re(conj w^ N^), T_E with 1 / |k|^2, T_theta(s) = sum Re(conj theta^ N_theta^)
        (None without a scalar), N^ the step's dealiased nonlinear term evaluated once in the co-moving frame (the mean flow transfers nothing)
        and, for the scalar, advection alone (no mean gradient).  Each sums to zero over the shells, to float32 rounding.  Uses ``state.work``;
        leaves what, that, mean and steps untouched."""
        self._state(state)
        out = ops.spec_ns_transfer(state.what, state.that, state.work, self.ny, self.Lx, self.Ly)
        return Transfer(self.shells()[0], out[:, 0], out[:, 1], None if state.that is None else out[:, 2])

    def energy_budget(self, state):
        """dE(s)/dt = T_E(s) + F(s) - 2 nu Z(s) - 2 drag E(s), float64 [B, S]: the right-hand side of the energy equation per shell (the
        viscous term is exact per shell: |k|^2 E_mode = Z_mode); for a buoyant state plus ``buoyancy_spectrum``.  With a stochastic force it adds
        ``stochastic_injection()``, the MEAN rate of that force (the same for every grid): the budget of the expectation, not of one realisation.
        With hyperviscosity, hypofriction or beta the linear terms are D_E(s) of ``linear_spectrum``: dE(s)/dt = T_E(s) + F(s) + D_E(s) (+ ...)."""
        sp, tr = self.spectrum(state), self.transfer(state)
        if self._linear():
            rhs = tr.energy + sp.injection + self.linear_spectrum(state).energy
        else:
            rhs = tr.energy + sp.injection - 2.0 * self.nu * sp.enstrophy - 2.0 * self.drag * sp.energy
        if self.stoch_amp is not None:
            rhs = rhs + torch.from_numpy(self.stochastic_injection()).to(rhs.device)
        return rhs + self.buoyancy_spectrum(state) if self._buoyant(state) else rhs

    def buoyancy_power(self, state):
        """b . <u theta'> = bx flux_x + by flux_y of ``scalar_diagnostics``, float64 [B]: the rate at which buoyancy feeds the fluctuation
        energy (zeros with b = (0, 0))."""
        d = self.scalar_diagnostics(state)
        return self.buoyancy[0] * d.flux_x + self.buoyancy[1] * d.flux_y

    def buoyancy_spectrum(self, state):
        """``buoyancy_power`` by wavenumber shell (``shells()``), float64 [B, S], summed on the device in the fixed order of ``spectrum``; its
        sum over the shells is ``buoyancy_power``.  Only reads the state."""
        self._scalar_state(state)
        return ops.spec_ns_buoyancy_spectrum(state.what, state.that, self.ny, self.Lx, self.Ly, self.buoyancy)

    def fields(self, state, out=None):
        """(u, v, p) float32 [B, nx, ny] of the state (into ``out`` if given); p includes the buoyancy's part for a buoyant state."""
        self._state(state)
        if self._buoyant(state):
            return ops.spec_ns_fields_buoyant(state.what, state.that, state.mean, state.work, self.ny, self.Lx, self.Ly, self.rho, self.buoyancy,
                                              out)
        return ops.spec_ns_fields(state.what, state.mean, state.work, self.ny, self.Lx, self.Ly, self.rho, out)

    # ---- Lagrangian tracers
    @staticmethod
    def _spline_order(order):
        order = _int('order', order)
        if order not in (4, 6):
            raise ValueError("order = %d must be 4 (cubic B-splines) or 6 (quintic)" % order)
        return order

    def init_particles(self, x, y, order=4, batch=None, device=None):
        """PeriodicParticles at (x, y): [B, P] each, or [P] shared by ``batch`` grids (default 1); numpy or torch of any float dtype, kept
        as float64.  Positions need not lie in the box.  ``order``: 4 or 6, the B-spline order every read of the flow at them uses."""
        order = self._spline_order(order)
        was_cuda = [a.device for a in (x, y) if isinstance(a, torch.Tensor) and a.is_cuda]
        dev = was_cuda[0] if was_cuda else _device(device)
        x, y = (torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(dtype=torch.float64, device=dev) for a in (x, y))
        if x.shape != y.shape or x.dim() not in (1, 2) or x.shape[-1] < 1:
            raise ValueError("init_particles: x and y must share the shape [B, P] or [P], got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        if x.dim() == 1:
            B = 1 if batch is None else _count('batch', batch, 1)
            x, y = x.expand(B, -1), y.expand(B, -1)
        elif batch is not None and _count('batch', batch, 1) != x.shape[0]:
            raise ValueError("init_particles: batch = %d, the positions are for %d grids" % (batch, x.shape[0]))
        return PeriodicParticles(torch.stack([x, y], dim=-1).contiguous(), order, (self.Lx, self.Ly), (self.nx, self.ny))

    def _own_particles(self, particles):
        if not isinstance(particles, PeriodicParticles):
            raise TypeError("PeriodicParticles (from init_particles) expected, got %s" % type(particles).__name__)
        if particles.grid != (self.nx, self.ny) or particles.box != (self.Lx, self.Ly):
            raise ValueError("particles of another solver: grid %s, box %s" % (particles.grid, particles.box))
        return particles

    def _particles(self, particles, state):
        self._own_particles(particles)
        if particles.batch != state.batch:
            raise ValueError("the particles are for %d grids, the state has %d" % (particles.batch, state.batch))
        if particles.pos.device != state.what.device:
            raise ValueError("the particles are on %s, the state on %s" % (particles.pos.device, state.what.device))
        return particles

    def _field_mask(self, fields, state):
        """(mask, slots): the C entry's field mask and, per requested name, its image's index among the mask's."""
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        if not fields:
            raise ValueError("fields must name at least one of %s" % (ops.PARTICLE_FIELDS,))
        for f in fields:
            if f not in ops.PARTICLE_FIELDS:
                raise ValueError("field %r is not one of %s" % (f, ops.PARTICLE_FIELDS))
        if 'theta' in fields and state.that is None:
            raise ValueError("field 'theta': the state carries no scalar")
        bits = sorted(set(ops.PARTICLE_FIELDS.index(f) for f in fields))
        return sum(1 << b for b in bits), [bits.index(ops.PARTICLE_FIELDS.index(f)) for f in fields]

    def _coefficients(self, state, mask, order, coef=None, work=None):
        nf, B = bin(mask).count('1'), state.batch
        if coef is None:
            coef = torch.empty((nf, B, self.nx, self.ny), dtype=torch.float32, device=state.what.device)
            work = torch.empty(ops.spec_ns_particle_workspace(B, nf, self.nx, self.ny), dtype=torch.uint8, device=state.what.device)
        return ops.spec_ns_particle_coefs(state.what, state.that if mask & 8 else None, state.mean, coef, mask, order, work, self.ny, self.Lx,
                                          self.Ly)

    def particle_coefficients(self, state, fields=('u', 'v'), order=4):
        """The B-spline coefficients of ``fields`` (names among 'u', 'v', 'w', 'theta'), a tuple of float32 [B, nx, ny] tensors in that order:
        c = irfft2(f^ / (beta_x beta_y)), the class note's prefilter.  For tests and for samplers of the user's own."""
        self._state(state)
        mask, slots = self._field_mask(fields, state)
        coef = self._coefficients(state, mask, self._spline_order(order))
        return tuple(coef[s] for s in slots)

    def sample(self, state, particles, fields=('u', 'v')):
        """float32 [B, P, len(fields)]: ``fields`` of the state at the particles' positions, by B-splines of the particles' order."""
        self._state(state)
        self._particles(particles, state)
        mask, slots = self._field_mask(fields, state)
        out = ops.spec_ns_particle_sample(self._coefficients(state, mask, particles.order), particles.pos, particles.order, self.Lx, self.Ly)
        return out if slots == list(range(out.shape[-1])) else out[..., slots].contiguous()

    # ---- reverse mode of the sampling
    def sample_gradient(self, state, particles, fields=('u', 'v')):
        """float32 [B, P, len(fields), 2]: (d/dx, d/dy) of ``fields`` at the particles, the exact derivative of the spline that ``sample``
        evaluates -- for (u, v) the velocity-gradient tensor at the particle: strain, Okubo-Weiss, the tangent of a trajectory.  The gather
        of ``sample`` with derivative weights on one axis (include/nns.h: nns_spec_ns_particle_sample_grad_f32); one lane per particle, a
        fixed order of summation, no atomics.  A spline of order 4 (6) is C^2 (C^4): the derivative is continuous across cells, and one
        order less accurate than the value."""
        self._state(state)
        self._particles(particles, state)
        mask, slots = self._field_mask(fields, state)
        out = ops.spec_ns_particle_sample_grad(self._coefficients(state, mask, particles.order), particles.pos, particles.order, self.Lx, self.Ly)
        return out if slots == list(range(out.shape[2])) else out[:, :, slots].contiguous()

    def particle_cells(self, particles):
        """(perm, start): the particles sorted by the cell that ``sample`` finds them in.  perm, int64 [B P]: the particle (an index into the
        flattened [B, P]) of every sorted slot, the particles of one cell in ascending index; start, int32 [B nx ny + 1]: the first slot
        of cell (b nx + ci) ny + cj, and B P last, so that cell k holds perm[start[k] : start[k + 1]].  One launch, a stable torch.sort and
        a torch.searchsorted on the device; no host synchronisation.  The positions are not reordered."""
        p = self._own_particles(particles)
        return ops.spec_ns_particle_cells(p.pos, self.nx, self.ny, self.Lx, self.Ly)

    def spread(self, particles, values):
        """A tuple of C float32 [B, nx, ny] images from ``values``, float32 device tensor [B, P, C] with C <= 4: image c holds, at node
        (i0 + a, j0 + c'), the sum over the particles of wx[a] wy[c'] values[b, p, c] -- the exact transpose of the gather that ``sample``
        applies to ``particle_coefficients``, sum(sample-gather(C) . r) = sum(C . spread(r)).  Point forces, binning, the backward of
        ``observe``.  A gather over the particles sorted by cell (``particle_cells``), float64 sums in a fixed order, no atomics: it repeats
        bitwise and a grid does not depend on its batch neighbours; nodes that no particle reaches are exactly 0."""
        p = self._own_particles(particles)
        if not (isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.float32 and values.dim() == 3):
            raise TypeError("spread: values must be a float32 device tensor [B, P, C]")
        if tuple(values.shape[:2]) != (p.batch, p.count) or not 1 <= values.shape[2] <= 4 or values.device != p.pos.device:
            raise ValueError("spread: values must be [%d, %d, C <= 4] on %s, got %s on %s"
                             % (p.batch, p.count, p.pos.device, tuple(values.shape), values.device))
        perm, start = ops.spec_ns_particle_cells(p.pos, self.nx, self.ny, self.Lx, self.Ly)
        out = ops.spec_ns_particle_spread(values.contiguous(), p.pos, perm, start, self.nx, self.ny, p.order, self.Lx, self.Ly)
        return tuple(out[c] for c in range(out.shape[0]))

    def observe(self, w, x, y, fields=('u', 'v'), theta=None, mean=None, order=4):
        """float32 [B, P, len(fields)]: ``fields`` (names among 'u', 'v', 'w', 'theta') of the vorticity field w (float32 device tensor
        [B, nx, ny] or [nx, ny]; ``theta`` likewise, on a solver with ``kappa``) read at the points (x, y), float64 device tensors [B, P], or
        [P] shared by the batch -- one autograd node, differentiable in w, theta, x and y, so that
        ``loss(observe(evolve(w0, n), x, y))`` reaches w0, theta0, the forcing and the operator table through ``evolve``, and the
        positions.  The forward is bitwise ``sample(init_vorticity(w, mean), init_particles(x, y, order), fields)``.  The backward into w
        and theta is the transpose of that chain: ``particle_cells``, ``spread``, the coefficient build's transpose (the forward's Fourier
        multipliers conjugated, one transform per field), then ``vorticity`` / ``scalar``; into x and y the cotangent times
        ``sample_gradient``, summed over the fields in float64 (over the grids too for shared positions).  No atomics anywhere: gradients
        repeat bitwise.  ``mean``: the mean velocity of u and v, a constant that gets no cotangent, as in ``evolve``."""
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        w = self._grad_field('w', w)
        if theta is not None:
            if self.kappa is None:
                raise ValueError("observe: theta needs a solver built with kappa (the scalar's diffusivity)")
            theta = self._grad_field('theta', theta)
            if theta.shape != w.shape or theta.device != w.device:
                raise ValueError("observe: w and theta must share their shape and device")
        elif 'theta' in fields:
            raise ValueError("observe: field 'theta' needs theta%s" % ("" if self.kappa is not None else " and a solver built with kappa"))
        for name, a in (('x', x), ('y', y)):
            if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float64):
                raise TypeError("observe: %s must be a float64 device tensor [B, P] or [P]" % name)
        if x.shape != y.shape or x.dim() not in (1, 2) or x.device != w.device:
            raise ValueError("observe: x and y must share the shape [B, P] or [P] on the field's device, got %s and %s"
                             % (tuple(x.shape), tuple(y.shape)))
        return _ObserveFn.apply(_Look(self, fields, mean, self._spline_order(order)), w, theta, x, y)

    def advect(self, state, particles, nsteps, scheme='rk4'):
        """``nsteps`` steps of the flow and of the particles in it, both in place; returns (state, particles).  The state goes through
        ``step``'s own launches one step at a time and comes out bitwise as from ``step(state, nsteps)``.  scheme 'rk4': classical RK4 of
        step 2 dt over pairs of flow steps (``nsteps`` even), 'heun': second order, any ``nsteps``; see the class note.  One coefficient
        build and two particle launches per flow step between the step's launches: no allocation, no host synchronisation, no torch
        operation, capturable on one stream.  n steps in one call are bitwise n / 2 calls of 2 steps."""
        self._state(state)
        p = self._particles(particles, state)
        nsteps = _count('nsteps', nsteps, 0)
        if scheme not in ('rk4', 'heun'):
            raise ValueError("scheme = %r must be 'rk4' or 'heun'" % (scheme,))
        if scheme == 'rk4' and nsteps % 2:
            raise ValueError("scheme 'rk4' advances the particles over pairs of flow steps: nsteps = %d must be even" % nsteps)
        if nsteps == 0:
            return state, particles
        self._force_of(state)
        dt, box = self.dt, (p.order, self.Lx, self.Ly)
        build = lambda k: self._coefficients(state, 3, p.order, p._coef[k], p._work)
        stage = lambda k, pos_in, pos_out, a, wk, c, first, closing: ops.spec_ns_particle_stage_(
            p._coef[k], p.pos, pos_in, pos_out, p._acc, a, wk, c, first, closing, *box)
        cur = 0                                                # p._coef[cur]: the flow at the start of the step
        build(cur)
        if scheme == 'rk4':
            for _ in range(nsteps // 2):
                stage(cur, p.pos, p._stage, dt, 1.0, 0.0, True, False)
                self._launch_steps(state, 1)
                build(1 - cur)
                stage(1 - cur, p._stage, p._stage, dt, 2.0, 0.0, False, False)
                stage(1 - cur, p._stage, p._stage, 2.0 * dt, 2.0, 0.0, False, False)
                self._launch_steps(state, 1)
                build(cur)
                stage(cur, p._stage, p.pos, 0.0, 1.0, dt / 3.0, False, True)
        else:
            for _ in range(nsteps):
                stage(cur, p.pos, p._stage, dt, 1.0, 0.0, True, False)
                self._launch_steps(state, 1)
                cur = 1 - cur
                build(cur)
                stage(cur, p._stage, p.pos, 0.0, 1.0, 0.5 * dt, False, True)
        state.steps += nsteps
        return state, particles

    def simulate(self, u0, v0, nsteps, save_every=1, use_graph=None, theta0=None):
        """Frames (U, V, P), each float32 [T, B, nx, ny] with T = nsteps // save_every + 1: the projected initial condition, then every
        save_every-th step; with ``theta0`` (U, V, P, Theta), the scalar's frames as well.  By default one step is captured as a HIP graph and replayed (use_graph=False: the eager loop; a capture that
        fails falls back to it); same kernels in the same order, so the frames are bitwise those of the eager loop."""
        nsteps, save_every = _count('nsteps', nsteps, 0), _count('save_every', save_every, 1)
        if nsteps % save_every:
            raise ValueError("nsteps = %d is not a multiple of save_every = %d" % (nsteps, save_every))
        state = self.init(u0, v0, theta0)
        self._force_of(state)
        T = nsteps // save_every + 1
        U = torch.empty((T, state.batch, self.nx, self.ny), dtype=torch.float32, device=state.what.device)
        V, P = torch.empty_like(U), torch.empty_like(U)
        Theta = None if theta0 is None else torch.empty_like(U)

        def save(k):
            self.fields(state, out=(U[k], V[k], P[k]))
            if Theta is not None:
                self.scalar(state, out=Theta[k])
        save(0)
        if use_graph is None:
            use_graph = True
        graph = None
        if use_graph and nsteps > 0:
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):                       # first launches (code-object load, LDS attributes) outside the capture
                    scratch = state.clone()
                    self.step(scratch, 1)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    self._launch_steps(state, 1)
            except Exception as e:                                   # noqa: BLE001 -- the eager loop is the same computation
                print('PeriodicSolver: HIP graph capture of the step failed (%r): running eagerly' % (e,))
                graph = None
        self.last_simulate_used_graph = graph is not None
        for k in range(1, T):
            if graph is not None:
                for _ in range(save_every):
                    graph.replay()
                state.steps += save_every
            else:
                self.step(state, save_every)
            save(k)
        return (U, V, P) if Theta is None else (U, V, P, Theta)

    def residual_engine(self, backend='spectral', precise=True, every=1):
        """A ResidualEngine with this solver's constants, for frames ``every`` steps apart (its dt = every * dt).  The engine knows neither
        force nor drag: on the frames of a forced run its momentum residuals converge (as dt -> 0) to f_s - drag (u - <u>), the right-hand
        side of the class note, rather than to zero; subtract that (``forcing_fields``) to measure the discretisation alone.  Likewise on
        buoyant frames the momentum residual converges to b theta' (plus the forced terms), theta' = ``scalar`` minus its grid mean, and on
        frames of a run with hyperviscosity, hypofriction or beta to those extra linear terms: -(nu_h (-lap)^p + mu (-lap)^-q) (u - <u>) and
        the solenoidal part of (0, beta psi), psi the streamfunction (u = psi_y, v = -psi_x), the force whose curl is -beta v'."""
        every = _count('every', every, 1)
        return ResidualEngine(self.nx, self.ny, self.dt * every, self.rho, self.nu, self.Lx, self.Ly, backend=backend, precise=precise)
