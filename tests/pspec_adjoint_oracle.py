"""NumPy float64 restatement (tests only) of the reverse mode of the forced Lawson RK4 step of the pseudo-spectral periodic solver
(csrc/pspec_kernels.hip: nns_spec_ns_step_adjoint_f32; nns.periodic.PeriodicSolver.advance): tests/pspec_forced_oracle.py plus its
vector-Jacobian product.

Cotangents are real band-limited fields paired by the plain grid sum <a, b> = sum a b and kept as their rfft2 spectra (unnormalised, the
layout of w^), so the multipliers E and M, real and even in k, are their own adjoints and no half-spectrum weight appears.

    N(w) = -M (u w_x + v w_y) + g,      u = psi_y + U0,  v = -psi_x + V0,  psi^ = w^ / |k|^2
    N'(s)^T kappa = M [u kappa_x + v kappa_y] + lap^-1 M [kappa_x w_y - kappa_y w_x]          (u, v, w_x, w_y of the stage state s)

(the first term: u is divergence-free, so -(u . grad)^T = u . grad; the second: delta u = curl^-1 delta w moved onto kappa grad w; in spectra
lap^-1 is -1 / |k|^2).  With s0 = w, s1 = E (w + dt/2 a), s2 = E w + dt/2 b, s3 = E^2 w + dt E c and lam the cotangent of w+:

    k4 = dt/6 lam                         r = N'(s3)^T k4      wbar  = E^2 lam + E^2 r
    k3 = dt/3 E lam + dt E r              r = N'(s2)^T k3      wbar += E r
    k2 = dt/3 E lam + dt/2 r              r = N'(s1)^T k2      wbar += E r
    k1 = dt/6 E^2 lam + dt/2 E r          r = N'(s0)^T k1      wbar += r
    gbar = k1 + k2 + k3 + k4

The mean flow is a constant of the step and is not differentiated.
"""
import numpy as np

import pspec_forced_oracle as F

WRONG = ('no_inverse_laplacian', 'stage_shift', 'no_E_in_k3', 'no_mean_flow')


class AdjointScheme(F.ForcedScheme):
    """wrong: None, or one of WRONG -- a deliberately wrong reverse mode (mutation tests): the lap^-1 term dropped, the stage states shifted
    by one (s0, s0, s1, s2 where s0, s1, s2, s3 belong), the factor E missing from k3 (k3 = dt/3 lam + dt r), the mean flow left out of u, v."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, wrong=None):
        F.ForcedScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag)
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.wrong = wrong

    def rfft2(self, f):
        return np.fft.rfft2(f)

    def pair(self, a, b):
        """<a, b> per grid of two spectra of real fields: the grid sum of the product of the fields."""
        return (self.irfft2(a) * self.irfft2(b)).sum(axis=(-2, -1))

    def nonlinear_vjp(self, w, mean, kappa):
        if self.wrong == 'no_mean_flow':
            mean = np.zeros_like(mean)
        kappa = self.M * kappa
        uh, vh = self.velocity_hat(w, mean)
        u, v = self.irfft2(uh), self.irfft2(vh)
        wx, wy = self.irfft2(1j * self.kx * w), self.irfft2(1j * self.ky * w)
        kx_, ky_ = self.irfft2(1j * self.kx * kappa), self.irfft2(1j * self.ky * kappa)
        q1 = self.rfft2(u * kx_ + v * ky_)
        q2 = self.rfft2(kx_ * wy - ky_ * wx)
        if self.wrong == 'no_inverse_laplacian':
            return self.M * q1
        return self.M * (q1 - q2 * self.ik2)

    def stages(self, w, mean):
        """(s0, s1, s2, s3) of one step from w."""
        dt = self.dt
        lam = self.nu * self.k2 + self.drag
        E, E2 = np.exp(-lam * dt / 2), np.exp(-lam * dt)
        a = self.nonlinear(w, mean, 1)
        s1 = E * (w + dt / 2 * a)
        b = self.nonlinear(s1, mean, 2)
        s2 = E * w + dt / 2 * b
        c = self.nonlinear(s2, mean, 3)
        s3 = E2 * w + dt * E * c
        return w, s1, s2, s3

    def step_vjp(self, w, mean, lam, nsteps=1):
        """(wbar, gbar): the cotangents of the start spectrum w and of the source g^ (one per grid, summed over the steps) for the cotangent
        lam of the spectrum after nsteps steps from w."""
        dt = self.dt
        rate = self.nu * self.k2 + self.drag
        E, E2 = np.exp(-rate * dt / 2), np.exp(-rate * dt)
        starts = []
        for _ in range(nsteps):
            starts.append(w)
            w = self.step(w, mean, 1)
        lam = self.M * np.asarray(lam, dtype=np.complex128)
        gbar = np.zeros_like(lam)
        for w0 in reversed(starts):
            s0, s1, s2, s3 = self.stages(w0, mean)
            if self.wrong == 'stage_shift':
                s0, s1, s2, s3 = s0, s0, s1, s2
            k4 = dt / 6 * lam
            r = self.nonlinear_vjp(s3, mean, k4)
            wbar = E2 * lam + E2 * r
            k3 = dt / 3 * lam + dt * r if self.wrong == 'no_E_in_k3' else dt / 3 * E * lam + dt * E * r
            r = self.nonlinear_vjp(s2, mean, k3)
            wbar = wbar + E * r
            k2 = dt / 3 * E * lam + dt / 2 * r
            r = self.nonlinear_vjp(s1, mean, k2)
            wbar = wbar + E * r
            k1 = dt / 6 * E2 * lam + dt / 2 * E * r
            r = self.nonlinear_vjp(s0, mean, k1)
            wbar = wbar + r
            gbar = gbar + k1 + k2 + k3 + k4
            lam = wbar
        return lam, gbar

    # ---- the ends of advance_velocity: init and the velocity part of fields, and their adjoints
    def velocity(self, w, mean):
        uh, vh = self.velocity_hat(w, mean)
        return self.irfft2(uh), self.irfft2(vh)

    def velocity_vjp(self, ubar, vbar):
        """K^T(ubar, vbar)^ = curl(ubar, vbar)^ / |k|^2 on the band: the cotangent of w^ for the cotangents (fields) of u, v = velocity(w)."""
        uh, vh = self.rfft2(ubar), self.rfft2(vbar)
        return self.M * (1j * self.kx * vh - 1j * self.ky * uh) * self.ik2

    def init_vjp(self, lam):
        """init^T(lam) = (lam_y, -lam_x) as fields: the cotangents of (u0, v0) for the cotangent lam of w^ = init(u0, v0)."""
        lam = self.M * lam
        return self.irfft2(1j * self.ky * lam), -self.irfft2(1j * self.kx * lam)
