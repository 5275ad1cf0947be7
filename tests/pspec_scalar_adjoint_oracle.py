"""NumPy float64 restatement (tests only) of the reverse mode of the scalar and the buoyant Lawson RK4 step of the pseudo-spectral periodic
solver (csrc/pspec_kernels.hip: nns_spec_ns_step_scalar_adjoint_f32; nns.periodic.PeriodicSolver.advance_scalar / advance_velocity_scalar):
tests/pspec_buoyant_oracle.py plus its vector-Jacobian product.

The state is z = (w^, theta^).  Cotangents are real band-limited fields paired by the plain grid sum <a, b> = sum a b and kept as their rfft2
spectra (unnormalised, the layout of w^), as in tests/pspec_adjoint_oracle.py.

    N_w     = -M (u w_x + v w_y)^ + g^ + M (i kx by - i ky bx) theta^
    N_theta = -M_theta (u (theta_x + Gx) + v (theta_y + Gy))^                                        (M_theta keeps the (0, 0) mode)

With kappa the cotangent of a stage's N_w, m that of its N_theta, and u, v (means included), w, theta of the stage state:

    r_w     = M [u kappa_x + v kappa_y]^ + lap^-1 M [kappa_x w_y - kappa_y w_x + m_x (theta_y + Gy) - m_y (theta_x + Gx)]^
    r_theta = M_theta [u m_x + v m_y - by kappa_x + bx kappa_y]^

(the scalar's advection is transposed like the vorticity's: u is divergence-free; delta u = curl^-1 delta w reaches N_theta as it reaches N_w,
which puts m grad(theta + G . x) beside kappa grad w under the inverse Laplacian; the buoyancy i k x b is antisymmetric, so its transpose is
-(by kappa_x - bx kappa_y)).  The Lawson recurrences are the parent's, with E = exp(-(nu |k|^2 + drag) dt / 2) on (lam, kappa, r_w, wbar) and
E_theta = exp(-kappa_diff |k|^2 dt / 2), no drag, on (mu, m, r_theta, thetabar):

    k4 = dt/6 lam                    m4 = dt/6 mu                                (r_w, r_theta) at s3    wbar  = E^2 (lam + r_w)    thetabar  = E_theta^2 (mu + r_theta)
    k3 = dt/3 E lam + dt E r_w       m3 = dt/3 E_theta mu + dt E_theta r_theta   at s2                   wbar += E r_w              thetabar += E_theta r_theta
    k2 = dt/3 E lam + dt/2 r_w       m2 = dt/3 E_theta mu + dt/2 r_theta         at s1                   wbar += E r_w              thetabar += E_theta r_theta
    k1 = dt/6 E^2 lam + dt/2 E r_w   m1 = dt/6 E_theta^2 mu + dt/2 E_theta r_theta   at s0               wbar += r_w                thetabar += r_theta
    gbar = k1 + k2 + k3 + k4         (the vorticity source, summed over steps)

The mean flow, G, b, kappa_diff, nu and the drag are constants and are not differentiated.
"""
import numpy as np

import pspec_buoyant_oracle as BO

WRONG = ('no_mu_in_wbar', 'no_gradient', 'buoyancy_sign', 'no_buoyancy_adjoint', 'scalar_dragged', 'stage_shift')


class ScalarAdjointScheme(BO.BuoyantScheme):
    """wrong: None, or one of WRONG -- a deliberately wrong reverse mode (mutation tests): the m terms dropped from the lap^-1 product, G dropped
    there, the sign of the buoyancy's adjoint flipped, that adjoint left out, E_theta with the drag, both stage states shifted by one
    (s0, s0, s1, s2 where s0, s1, s2, s3 belong)."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, kappa=0.0, grad=(0.0, 0.0), buoy=(0.0, 0.0), wrong=None):
        BO.BuoyantScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, kappa=kappa, grad=grad, buoy=buoy)
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.wrong = wrong

    def rfft2(self, f):
        return np.fft.rfft2(f)

    def pair(self, a, b):
        """<a, b> per grid of two spectra of real fields: the grid sum of the product of the fields."""
        return (self.irfft2(a) * self.irfft2(b)).sum(axis=(-2, -1))

    def nonlinear_vjp(self, w, t, mean, kappa, m):
        """(r_w, r_theta) for the cotangents (kappa, m) of (N_w, N_theta) at the state (w, t)."""
        kappa, m = self.M * kappa, self.Mt * m
        uh, vh = self.velocity_hat(w, mean)
        u, v = self.irfft2(uh), self.irfft2(vh)
        d = lambda f: (self.irfft2(1j * self.kx * f), self.irfft2(1j * self.ky * f))
        (wx, wy), (tx, ty), (kx_, ky_), (mx_, my_) = d(w), d(t), d(kappa), d(m)
        gx, gy = (0.0, 0.0) if self.wrong == 'no_gradient' else self.grad
        bx, by = self.buoy
        if self.wrong == 'buoyancy_sign':
            bx, by = -bx, -by
        elif self.wrong == 'no_buoyancy_adjoint':
            bx, by = 0.0, 0.0
        q2 = kx_ * wy - ky_ * wx
        if self.wrong != 'no_mu_in_wbar':
            q2 = q2 + mx_ * (ty + gy) - my_ * (tx + gx)
        r_w = self.M * (self.rfft2(u * kx_ + v * ky_) - self.rfft2(q2) * self.ik2)
        r_t = self.Mt * self.rfft2(u * mx_ + v * my_ - by * kx_ + bx * ky_)
        return r_w, r_t

    def factors(self):
        """(E, E^2, E_theta, E_theta^2) of the reverse mode."""
        dt = self.dt
        lw = self.nu * self.k2 + self.drag
        lt = self.kappa * self.k2 + (self.drag if self.wrong == 'scalar_dragged' else 0.0)
        return np.exp(-lw * dt / 2), np.exp(-lw * dt), np.exp(-lt * dt / 2), np.exp(-lt * dt)

    def stages(self, w, t, mean):
        """((w, t) of s0, s1, s2, s3) of one step from (w, t): the statements of BuoyantScheme.step."""
        dt = self.dt
        lw, lt = self.nu * self.k2 + self.drag, self.kappa * self.k2
        E, E2, Et, Et2 = np.exp(-lw * dt / 2), np.exp(-lw * dt), np.exp(-lt * dt / 2), np.exp(-lt * dt)
        a, at = self.nonlinear_w(w, t, mean, 1), self.nonlinear_scalar(w, t, mean)
        w2, t2 = E * (w + dt / 2 * a), Et * (t + dt / 2 * at)
        b, bt = self.nonlinear_w(w2, t2, mean, 2), self.nonlinear_scalar(w2, t2, mean)
        w3, t3 = E * w + dt / 2 * b, Et * t + dt / 2 * bt
        c, ct = self.nonlinear_w(w3, t3, mean, 3), self.nonlinear_scalar(w3, t3, mean)
        w4, t4 = E2 * w + dt * E * c, Et2 * t + dt * Et * ct
        return (w, t), (w2, t2), (w3, t3), (w4, t4)

    def step_vjp(self, w, t, mean, lam, mu, nsteps=1):
        """(wbar, thetabar, gbar): the cotangents of the start spectra (w, t) and of the vorticity source g^ (one per grid, summed over the
        steps) for the cotangents (lam, mu) of the spectra after nsteps steps from (w, t)."""
        dt = self.dt
        E, E2, Et, Et2 = self.factors()
        starts = []
        for _ in range(nsteps):
            starts.append((w, t))
            w, t = self.step(w, t, mean, 1)
        lam = self.M * np.asarray(lam, dtype=np.complex128)
        mu = self.Mt * np.asarray(mu, dtype=np.complex128)
        gbar = np.zeros_like(lam)
        for w0, t0 in reversed(starts):
            s0, s1, s2, s3 = self.stages(w0, t0, mean)
            if self.wrong == 'stage_shift':
                s0, s1, s2, s3 = s0, s0, s1, s2
            k4, m4 = dt / 6 * lam, dt / 6 * mu
            rw, rt = self.nonlinear_vjp(s3[0], s3[1], mean, k4, m4)
            wbar, tbar = E2 * (lam + rw), Et2 * (mu + rt)
            k3, m3 = dt / 3 * E * lam + dt * E * rw, dt / 3 * Et * mu + dt * Et * rt
            rw, rt = self.nonlinear_vjp(s2[0], s2[1], mean, k3, m3)
            wbar, tbar = wbar + E * rw, tbar + Et * rt
            k2, m2 = dt / 3 * E * lam + dt / 2 * rw, dt / 3 * Et * mu + dt / 2 * rt
            rw, rt = self.nonlinear_vjp(s1[0], s1[1], mean, k2, m2)
            wbar, tbar = wbar + E * rw, tbar + Et * rt
            k1, m1 = dt / 6 * E2 * lam + dt / 2 * E * rw, dt / 6 * Et2 * mu + dt / 2 * Et * rt
            rw, rt = self.nonlinear_vjp(s0[0], s0[1], mean, k1, m1)
            wbar, tbar = wbar + rw, tbar + rt
            gbar = gbar + k1 + k2 + k3 + k4
            lam, mu = wbar, tbar
        return lam, mu, gbar

    # ---- the ends of advance_velocity_scalar: init and the velocity part of fields, and their adjoints (tests/pspec_adjoint_oracle.py's);
    # theta's ends, M_theta rfft2 and irfft2, are each other's transposes under the grid sum up to the mask
    def velocity(self, w, mean):
        uh, vh = self.velocity_hat(w, mean)
        return self.irfft2(uh), self.irfft2(vh)

    def velocity_vjp(self, ubar, vbar):
        uh, vh = self.rfft2(ubar), self.rfft2(vbar)
        return self.M * (1j * self.kx * vh - 1j * self.ky * uh) * self.ik2

    def init_vjp(self, lam):
        lam = self.M * lam
        return self.irfft2(1j * self.ky * lam), -self.irfft2(1j * self.kx * lam)
