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
(csrc/pspec_kernels.hip; scheme in DESIGN.md and tests/pspec_oracle.py).
"""
import math
import numbers

import numpy as np
import torch

from . import ops


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


def _pow2_axis(name, n):
    if isinstance(n, bool) or not isinstance(n, numbers.Integral):
        raise TypeError("%s must be an int, got %r" % (name, n))
    if not (64 <= n <= 1024 and n & (n - 1) == 0):
        raise ValueError("%s = %d: each axis must be a power of two in [64, 1024]" % (name, n))
    return int(n)


def _real(name, x, positive=True):
    if isinstance(x, bool) or not isinstance(x, numbers.Real):
        raise TypeError("%s must be a real number, got %r" % (name, x))
    x = float(x)
    if not math.isfinite(x) or (x <= 0 if positive else x < 0):
        raise ValueError("%s = %r must be finite and %s" % (name, x, "> 0" if positive else ">= 0"))
    return x


def _count(name, n, minimum):
    if isinstance(n, bool) or not isinstance(n, numbers.Integral):
        raise TypeError("%s must be an int, got %r" % (name, n))
    if n < minimum:
        raise ValueError("%s = %d must be >= %d" % (name, n, minimum))
    return int(n)


class PeriodicState(object):
    """State of a PeriodicSolver run; owns its device buffers.
    what: the vorticity spectrum, compacted to the kept y-wavenumbers and transposed (float32 [B, my1, nx, 2], include/nns.h: nns_spec_ns_*);
    mean: the conserved mean velocity (U0, V0) per grid, float32 [B, 2]; work: the solver's scratch; steps: steps taken since init."""

    def __init__(self, what, mean, work):
        self.what, self.mean, self.work = what, mean, work
        self.steps = 0

    @property
    def batch(self):
        return self.what.shape[0]

    def clone(self):
        """A copy with its own buffers (a fresh workspace: the solver keeps no data in it between calls)."""
        c = PeriodicState(self.what.clone(), self.mean.clone(), torch.empty_like(self.work))
        c.steps = self.steps
        return c


class PeriodicSolver(object):
    """Batched 2-D incompressible Navier-Stokes on the periodic box [0, Lx) x [0, Ly): float32 fields [B, nx, ny] on the device
    (axis 0 = x), nx and ny each a power of two in [64, 1024].  Vorticity-streamfunction form, 2/3-rule dealiasing
    (3|m_x| < nx and 3|m_y| < ny), integrating-factor (Lawson) RK4 in time; every step is HIP (csrc/pspec_kernels.hip), no FFT library.

    ``init(u, v)`` PROJECTS the input: the state keeps the vorticity of (u, v) inside the 2/3 band and the grid means (U0, V0), so
    ``fields(init(u, v))`` returns the divergence-free, band-limited part of (u, v) -- equal to it when (u, v) already is one.
    The mean velocity is conserved.  ``p`` is the pressure of the velocity field: lap p = 2 rho (u_x v_y - u_y v_x), zero mean."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * math.pi, Ly=2 * math.pi):
        self.nx, self.ny = _pow2_axis('nx', nx), _pow2_axis('ny', ny)
        self.dt, self.rho = _real('dt', dt), _real('rho', rho)
        self.nu = _real('nu', nu, positive=False)
        self.Lx, self.Ly = _real('Lx', Lx), _real('Ly', Ly)
        self.my1 = ops.spec_ns_kept_y(self.ny)
        self.last_simulate_used_graph = False

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
        return state

    def init(self, u, v):
        """State of velocity (u, v) ([B, nx, ny] or [nx, ny], float32): see the class note on the projection."""
        u, v = self._field('u', u), self._field('v', v)
        if u.shape != v.shape:
            raise ValueError("u and v must share their shape")
        from ._util import default_device
        dev = u.device if u.is_cuda else (v.device if v.is_cuda else default_device())
        u, v = u.to(dev).contiguous(), v.to(dev).contiguous()
        B = u.shape[0]
        what = torch.empty((B, self.my1, self.nx, 2), dtype=torch.float32, device=u.device)
        mean = torch.empty((B, 2), dtype=torch.float32, device=u.device)
        work = torch.empty(ops.spec_ns_workspace(B, self.nx, self.ny), dtype=torch.uint8, device=u.device)
        ops.spec_ns_init(u, v, what, mean, work, self.Lx, self.Ly)
        return PeriodicState(what, mean, work)

    def step(self, state, nsteps=1):
        """nsteps time steps in place (no allocation, no host synchronisation)."""
        self._state(state)
        nsteps = _count('nsteps', nsteps, 0)
        ops.spec_ns_step_(state.what, state.mean, state.work, self.ny, self.Lx, self.Ly, self.dt, self.nu, nsteps)
        state.steps += nsteps
        return state

    def fields(self, state, out=None):
        """(u, v, p) float32 [B, nx, ny] of the state (into ``out`` if given)."""
        self._state(state)
        return ops.spec_ns_fields(state.what, state.mean, state.work, self.ny, self.Lx, self.Ly, self.rho, out)

    def simulate(self, u0, v0, nsteps, save_every=1, use_graph=None):
        """Frames (U, V, P), each float32 [T, B, nx, ny] with T = nsteps // save_every + 1: the projected initial condition, then every
        save_every-th step.  By default one step is captured as a HIP graph and replayed (use_graph=False: the eager loop; a capture that
        fails falls back to it); same kernels in the same order, so the frames are bitwise those of the eager loop."""
        nsteps, save_every = _count('nsteps', nsteps, 0), _count('save_every', save_every, 1)
        if nsteps % save_every:
            raise ValueError("nsteps = %d is not a multiple of save_every = %d" % (nsteps, save_every))
        state = self.init(u0, v0)
        T = nsteps // save_every + 1
        U = torch.empty((T, state.batch, self.nx, self.ny), dtype=torch.float32, device=state.what.device)
        V, P = torch.empty_like(U), torch.empty_like(U)
        self.fields(state, out=(U[0], V[0], P[0]))
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
                    ops.spec_ns_step_(state.what, state.mean, state.work, self.ny, self.Lx, self.Ly, self.dt, self.nu, 1)
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
            self.fields(state, out=(U[k], V[k], P[k]))
        return U, V, P

    def residual_engine(self, backend='spectral', precise=True, every=1):
        """A ResidualEngine with this solver's constants, for frames ``every`` steps apart (its dt = every * dt)."""
        every = _count('every', every, 1)
        return ResidualEngine(self.nx, self.ny, self.dt * every, self.rho, self.nu, self.Lx, self.Ly, backend=backend, precise=precise)
