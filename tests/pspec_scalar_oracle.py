"""NumPy float64 restatement (tests only) of the passive scalar of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_scalar_f32, nns_spec_ns_scalar_*; nns.periodic.PeriodicSolver with kappa): tests/pspec_forced_oracle.py plus a scalar theta
[..., nx, ny] with diffusivity kappa >= 0 and a uniform mean gradient G = (Gx, Gy) -- the total field is G . x + theta, theta its periodic part:

    theta_t + u theta_x + v theta_y = kappa lap theta - (Gx u + Gy v)

State theta^ = M_theta rfft2(theta), M_theta = the 2/3 mask M with the (0, 0) mode KEPT (the mean of theta is state).  (w^, theta^) is ONE system
under the Lawson RK4 of the parent: L_theta = -kappa |k|^2 (the drag does not act on the scalar),
    N_theta(w^, theta^) = -M_theta rfft2(u (theta_x + Gx) + v (theta_y + Gy)),
u, v the stage's own velocity, means included; w^ evolves exactly as without the scalar.  Consequences:
    d<theta>/dt = -G . (U0, V0)   (the grid mean of u . grad theta is alias-free and zero),
    d/dt 1/2 <theta'^2> = -G . <u theta'> - kappa <|grad theta|^2>.
Diagnostics by Parseval over the half spectrum without its (0, 0) mode (weight 1 on m_y = 0, 2 on m_y > 0).
"""
import numpy as np

import pspec_forced_oracle as F
import pspec_oracle as O

MUTATIONS = ('nokappa', 'nograd', 'kappa_is_nu', 'dragged', 'frozen')


class ScalarScheme(F.ForcedScheme):
    """mutate: a deliberately wrong scheme (mutation tests) -- 'nokappa': kappa = 0; 'nograd': G ignored; 'kappa_is_nu': kappa replaced by nu;
    'dragged': the drag also damps theta; 'frozen': all four scalar stages use the stage-1 velocity.  widen reaches the scalar's nonlinear
    term through MN, as it reaches the vorticity's."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, kappa=0.0, grad=(0.0, 0.0), widen=(0, 0), mutate=None):
        F.ForcedScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, widen=widen)
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError("mutate must be None or one of %s" % (MUTATIONS,))
        self.kappa, self.grad, self.mutate = kappa, tuple(grad), mutate
        self.Mt, self.MNt = self.M.copy(), self.MN.copy()
        self.Mt[0, 0] = self.MNt[0, 0] = 1.0

    def init_scalar(self, theta):
        return self.Mt * np.fft.rfft2(np.asarray(theta, dtype=np.float64))

    def scalar_field(self, t):
        return self.irfft2(t)

    def nonlinear_scalar(self, w, t, mean):
        uh, vh = self.velocity_hat(w, mean)
        u, v = self.irfft2(uh), self.irfft2(vh)
        gx, gy = (0.0, 0.0) if self.mutate == 'nograd' else self.grad
        tx, ty = self.irfft2(1j * self.kx * t), self.irfft2(1j * self.ky * t)
        return -self.MNt * np.fft.rfft2(u * (tx + gx) + v * (ty + gy))

    def step(self, w, t, mean, nsteps=1):
        """(w, t) after nsteps steps; w goes through the statements of ForcedScheme.step, so it is that method's result bit for bit."""
        dt = self.dt
        lam = self.nu * self.k2 + self.drag
        E = np.exp(-lam * dt / 2)
        E2 = np.exp(-lam * dt)
        kappa = {'nokappa': 0.0, 'kappa_is_nu': self.nu}.get(self.mutate, self.kappa)
        lt = kappa * self.k2 + (self.drag if self.mutate == 'dragged' else 0.0)
        Et = np.exp(-lt * dt / 2)
        Et2 = np.exp(-lt * dt)
        frozen = self.mutate == 'frozen'
        for _ in range(nsteps):
            w1 = w
            a = self.nonlinear(w1, mean, 1)
            at = self.nonlinear_scalar(w1, t, mean)
            w2 = E * (w + dt / 2 * a)
            b = self.nonlinear(w2, mean, 2)
            bt = self.nonlinear_scalar(w1 if frozen else w2, Et * (t + dt / 2 * at), mean)
            w3 = E * w + dt / 2 * b
            c = self.nonlinear(w3, mean, 3)
            ct = self.nonlinear_scalar(w1 if frozen else w3, Et * t + dt / 2 * bt, mean)
            w4 = E2 * w + dt * E * c
            d = self.nonlinear(w4, mean, 4)
            dth = self.nonlinear_scalar(w1 if frozen else w4, Et2 * t + dt * Et * ct, mean)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
            t = Et2 * t + dt / 6 * (Et2 * at + 2 * Et * (bt + ct) + dth)
        return w, t

    def scalar_diag(self, w, t):
        """(variance 1/2 <theta'^2>, dissipation kappa <|grad theta|^2>, flux_x <u theta'>, flux_y <v theta'>), each [...], from the spectra alone."""
        wt = np.where(np.arange(self.ny // 2 + 1) == 0, 1.0, 2.0)[None, :]
        n2 = float(self.nx * self.ny) ** 2
        nz = (self.k2 > 0).astype(np.float64)
        t2 = wt * nz * (t.real ** 2 + t.imag ** 2)
        psi = w * self.ik2
        var = 0.5 * t2.sum(axis=(-2, -1)) / n2
        dis = self.kappa * (t2 * self.k2).sum(axis=(-2, -1)) / n2
        fx = (wt * nz * (1j * self.ky * psi * np.conj(t)).real).sum(axis=(-2, -1)) / n2
        fy = (wt * nz * (-1j * self.kx * psi * np.conj(t)).real).sum(axis=(-2, -1)) / n2
        return var, dis, fx, fy

    def fluctuation(self, t):
        """The spectrum without its (0, 0) mode."""
        t = np.array(t)
        t[..., 0, 0] = 0.0
        return t


def advected_sine(nx, ny, t, m, U, kappa, grad, c=0.0, Lx=2 * np.pi, Ly=2 * np.pi):
    """(theta, decayed amplitude) of theta(0) = sin(k . x) + c under the uniform flow U and the gradient G:
    theta = sin(k . (x - U t)) exp(-kappa |k|^2 t) + c - t G . U, k = 2 pi (m_x / Lx, m_y / Ly)."""
    kx, ky = 2 * np.pi * m[0] / Lx, 2 * np.pi * m[1] / Ly
    X, Y = np.meshgrid(Lx * np.arange(nx) / nx, Ly * np.arange(ny) / ny, indexing='ij')
    amp = np.exp(-kappa * (kx * kx + ky * ky) * t)
    return np.sin(kx * (X - U[0] * t) + ky * (Y - U[1] * t)) * amp + c - t * (grad[0] * U[0] + grad[1] * U[1]), amp
