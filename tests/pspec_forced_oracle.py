"""NumPy float64 restatement (tests only) of the forced, damped step of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_forced_f32, nns_spec_ns_diag_f32; nns.periodic.PeriodicSolver with drag / set_forcing): tests/pspec_oracle.py plus

    u_t + (u . grad) u = -grad p / rho + nu lap u - alpha (u - <u>) + f_s
    w_t + u w_x + v w_y = nu lap w - alpha w + g,      g^ = M (i kx f_y^ - i ky f_x^)

with f_s the solenoidal, zero-mean, band-limited part of a force f constant in time.  Lawson RK4 as there with
    L = -(nu |k|^2 + alpha),    N(w^) = -M rfft2(u w_x + v w_y) + g^   (the same g^ in all four stages).
The mean velocity stays conserved and undamped.  Diagnostics by Parseval over the half spectrum (weight 1 on m_y = 0, 2 on m_y > 0):
    E = 1/2 <|u - <u>|^2>,  Z = 1/2 <w^2>,  P = <f_s . u>,   dE/dt = P - 2 nu Z - 2 alpha E.
With no force and zero drag every method returns the parent's numbers exactly.
"""
import numpy as np

import pspec_oracle as O


class ForcedScheme(O.Scheme):
    """force_stages: the RK stages (1..4) whose nonlinear term gets g^; anything but all four is a deliberately wrong scheme (mutation tests)."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, widen=(0, 0), force_stages=(1, 2, 3, 4)):
        O.Scheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, widen=widen)
        self.drag = drag
        self.g = None
        self.force_stages = tuple(force_stages)

    def set_forcing(self, fx, fy=None):
        """g^ [..., nx, nh] of the force (fx, fy) [..., nx, ny] (leading axes broadcast against the state's); None removes it."""
        self.g = None if fx is None else self.init(fx, fy)[0]
        return self

    def kolmogorov_forcing(self, k=4, amplitude=1.0, dtype=np.float32):
        """f = (amplitude sin(2 pi k y / Ly), 0) [1, nx, ny], rounded to float32 as PeriodicSolver.kolmogorov_forcing hands it to the
        device (dtype=np.float64: the exact sine, for comparisons with analytic solutions below the float32 rounding)."""
        y = np.arange(self.ny) / float(self.ny)
        fx = np.broadcast_to(float(amplitude) * np.sin(2 * np.pi * int(k) * y), (1, self.nx, self.ny)).astype(dtype)
        return self.set_forcing(fx, np.zeros_like(fx))

    def forcing_fields(self):
        """(f_sx, f_sy): the part of the force that acts -- f_s is to g^ what the velocity is to w^."""
        u, v, _ = self.fields(self.g, np.zeros(self.g.shape[:-2] + (2,)))
        return u, v

    def nonlinear(self, w, mean, stage=1):
        n = O.Scheme.nonlinear(self, w, mean)
        return n if self.g is None or stage not in self.force_stages else n + self.g

    def step(self, w, mean, nsteps=1):
        dt = self.dt
        lam = self.nu * self.k2 + self.drag
        E = np.exp(-lam * dt / 2)
        E2 = np.exp(-lam * dt)
        for _ in range(nsteps):
            a = self.nonlinear(w, mean, 1)
            b = self.nonlinear(E * (w + dt / 2 * a), mean, 2)
            c = self.nonlinear(E * w + dt / 2 * b, mean, 3)
            d = self.nonlinear(E2 * w + dt * E * c, mean, 4)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
        return w

    def diag(self, w):
        """(E, Z, P), each [...]: fluctuation energy, enstrophy and power input from the spectrum w [..., nx, nh] alone."""
        wt = np.where(np.arange(self.ny // 2 + 1) == 0, 1.0, 2.0)[None, :]
        n2 = float(self.nx * self.ny) ** 2
        a2 = wt * (w.real ** 2 + w.imag ** 2)
        E = 0.5 * (a2 * self.ik2).sum(axis=(-2, -1)) / n2
        Z = 0.5 * a2.sum(axis=(-2, -1)) / n2
        if self.g is None:
            P = np.zeros_like(E)
        else:
            P = (wt * self.ik2 * (w * np.conj(self.g)).real).sum(axis=(-2, -1)) / n2
        return E, Z, P

    def expand(self, c):
        """The solver's state layout [..., my1, nx] (complex) -> rfft2 layout [..., nx, nh]: the inverse of compact."""
        w = np.zeros(c.shape[:-2] + (self.nx, self.ny // 2 + 1), dtype=np.complex128)
        w[..., :O.kept_y(self.ny)] = np.swapaxes(c, -1, -2)
        return w


def kolmogorov_laminar(nx, ny, t, A, k, lam, Ly=2 * np.pi, U0=0.0):
    """Kolmogorov flow from rest: f = (A sin(2 pi k y / Ly), 0), u(0) = (U0, 0): the advection term vanishes identically and
    u = U0 + A / lam (1 - exp(-lam t)) sin(2 pi k y / Ly), v = 0, p = 0, with lam = nu (2 pi k / Ly)^2 + alpha."""
    y = Ly * np.arange(ny) / ny
    u = U0 + A / lam * (-np.expm1(-lam * t)) * np.broadcast_to(np.sin(2 * np.pi * k * y / Ly), (nx, ny))
    return u, np.zeros((nx, ny)), np.zeros((nx, ny))
