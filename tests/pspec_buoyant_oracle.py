"""NumPy float64 restatement (tests only) of the Boussinesq buoyancy of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_buoyant_f32, nns_spec_ns_fields_buoyant_f32, nns_spec_ns_buoyancy_spectrum_f32; nns.periodic.PeriodicSolver with buoyancy):
tests/pspec_scalar_oracle.py plus the scalar acting on the flow through b theta', b = (bx, by) uniform, theta' = theta - <theta>:

    u_t + (u . grad) u = -grad p / rho + nu lap u - alpha (u - <u>) + f_s + b theta'
    w_t + u w_x + v w_y = nu lap w - alpha w + g + (by theta_x - bx theta_y)
    theta_t + u theta_x + v theta_y = kappa lap theta - G . u

Only the periodic fluctuation is buoyant: b <theta> would only accelerate the frame and the background G . x is taken as hydrostatic (its curl, a
constant, cannot exist on a periodic box).  (w^, theta^) is ONE system under the Lawson RK4 of the parents, the buoyancy explicit:
    N_w(w^, theta^) = -M rfft2(u w_x + v w_y) + g^ + M (i kx by - i ky bx) theta^,      theta^ each stage's own value;
L_w, L_theta and N_theta are unchanged.  Pressure: div(b theta') != 0, so lap p = rho (2 (u_x v_y - u_y v_x) + b . grad theta),
    p^ = p^ of the parent - rho i (k . b) theta^ / |k|^2 on the kept modes, zero mean.
Budgets: d/dt 1/2 <|u'|^2> = P - 2 nu Z - 2 alpha E + b . <u theta'>; for b = lambda G with nu = kappa = alpha = 0 and no force
E + lambda variance is conserved (d variance / dt = -G . <u theta'>).
"""
import numpy as np

import pspec_scalar_oracle as SO
import pspec_spectrum_oracle as PO

MUTATIONS = ('sign', 'swap', 'none', 'frozen', 'p_without_b')


class BuoyantScheme(SO.ScalarScheme):
    """mutate: a deliberately wrong scheme (mutation tests) -- 'sign': -b; 'swap': (by, bx); 'none': no buoyancy in the step; 'frozen': all four
    stages use the stage-1 theta^ in the buoyancy term; 'p_without_b': the pressure of the flow alone."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, kappa=0.0, grad=(0.0, 0.0), buoy=(0.0, 0.0), widen=(0, 0),
                 mutate=None):
        SO.ScalarScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, kappa=kappa, grad=grad, widen=widen)
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError("mutate must be None or one of %s" % (MUTATIONS,))
        self.buoy, self.bmutate = (float(buoy[0]), float(buoy[1])), mutate

    def buoyancy_hat(self, t):
        """M (i kx by - i ky bx) theta^: the buoyancy's term of the vorticity equation (None: nothing to add)."""
        bx, by = self.buoy
        if self.bmutate == 'sign':
            bx, by = -bx, -by
        elif self.bmutate == 'swap':
            bx, by = by, bx
        if self.bmutate == 'none' or (bx, by) == (0.0, 0.0):
            return None
        return self.MN * (1j * self.kx * by - 1j * self.ky * bx) * t

    def nonlinear_w(self, w, t, mean, stage):
        n, b = self.nonlinear(w, mean, stage), self.buoyancy_hat(t)
        return n if b is None else n + b

    def step(self, w, t, mean, nsteps=1):
        """(w, t) after nsteps steps of the coupled system; with b = 0 the statements of ScalarScheme.step, so that method's result bit for bit."""
        dt = self.dt
        lam = self.nu * self.k2 + self.drag
        E = np.exp(-lam * dt / 2)
        E2 = np.exp(-lam * dt)
        lt = self.kappa * self.k2
        Et = np.exp(-lt * dt / 2)
        Et2 = np.exp(-lt * dt)
        frozen = self.bmutate == 'frozen'
        for _ in range(nsteps):
            a = self.nonlinear_w(w, t, mean, 1)
            at = self.nonlinear_scalar(w, t, mean)
            w2, t2 = E * (w + dt / 2 * a), Et * (t + dt / 2 * at)
            b = self.nonlinear_w(w2, t if frozen else t2, mean, 2)
            bt = self.nonlinear_scalar(w2, t2, mean)
            w3, t3 = E * w + dt / 2 * b, Et * t + dt / 2 * bt
            c = self.nonlinear_w(w3, t if frozen else t3, mean, 3)
            ct = self.nonlinear_scalar(w3, t3, mean)
            w4, t4 = E2 * w + dt * E * c, Et2 * t + dt * Et * ct
            d = self.nonlinear_w(w4, t if frozen else t4, mean, 4)
            dth = self.nonlinear_scalar(w4, t4, mean)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
            t = Et2 * t + dt / 6 * (Et2 * at + 2 * Et * (bt + ct) + dth)
        return w, t

    def pressure_hat(self, w, mean, t):
        """p^ [..., nx, nh] of the buoyant flow."""
        uh, vh = self.velocity_hat(w, mean)
        ux, uy = self.irfft2(1j * self.kx * uh), self.irfft2(1j * self.ky * uh)
        vx, vy = self.irfft2(1j * self.kx * vh), self.irfft2(1j * self.ky * vh)
        p = -self.M * np.fft.rfft2(2 * self.rho * (ux * vy - uy * vx)) * self.ik2
        if self.bmutate != 'p_without_b':
            bx, by = self.buoy
            p = p - self.rho * 1j * (self.kx * bx + self.ky * by) * self.M * t * self.ik2
        return p

    def fields(self, w, mean, t=None):
        """(u, v, p); with theta^ given p is the buoyant pressure, without it the parent's."""
        u, v, p = SO.ScalarScheme.fields(self, w, mean)
        return (u, v, p) if t is None else (u, v, self.irfft2(self.pressure_hat(w, mean, t)))

    def poisson_residual(self, w, mean, t):
        """max |lap p - rho (2 (u_x v_y - u_y v_x) + b . grad theta')| over the grid, each side evaluated spectrally on the kept modes, relative
        to the max of the right-hand side."""
        uh, vh = self.velocity_hat(w, mean)
        ux, uy = self.irfft2(1j * self.kx * uh), self.irfft2(1j * self.ky * uh)
        vx, vy = self.irfft2(1j * self.kx * vh), self.irfft2(1j * self.ky * vh)
        bx, by = self.buoy
        tx, ty = self.irfft2(1j * self.kx * self.M * t), self.irfft2(1j * self.ky * self.M * t)
        rhs = self.irfft2(self.M * np.fft.rfft2(self.rho * (2 * (ux * vy - uy * vx) + bx * tx + by * ty)))
        lap = self.irfft2(-self.k2 * self.pressure_hat(w, mean, t))
        return np.abs(lap - rhs).max() / np.abs(rhs).max()

    def buoyancy_power(self, w, t):
        """b . <u theta'>, [...]: the buoyancy's term of the energy equation."""
        _, _, fx, fy = self.scalar_diag(w, t)
        return self.buoy[0] * fx + self.buoy[1] * fy

    def buoyancy_modes(self, w, t):
        """Re(conj(bx u^ + by v^) theta^) per mode, u^ = i ky psi^, v^ = -i kx psi^ (no mean: the (0, 0) mode contributes nothing)."""
        psi = w * self.ik2
        bu = self.buoy[0] * 1j * self.ky * psi - self.buoy[1] * 1j * self.kx * psi
        return (np.conj(bu) * t).real

    def buoyancy_spectrum(self, w, t):
        """B(s) [..., S]: buoyancy_power by the shells of tests/pspec_spectrum_oracle.py."""
        return PO.bin_shells(self, self.buoyancy_modes(w, t))


def plane_wave(nx, ny, t, m, b, G, U, nu, Lx=2 * np.pi, Ly=2 * np.pi):
    """The exact solution for a single wavevector k = 2 pi (m_x / Lx, m_y / Ly) with nu = kappa, at time t:
        psi = a(t) cos phi,  theta = c(t) sin phi - t G . U,  phi = k . (x - U t)
    (the nonlinear terms vanish identically), vorticity amplitude 1 at t = 0 (a0 = 1 / |k|^2):
        a = a0 exp(-nu |k|^2 t) cos(omega t),  c = -(k x G) a0 exp(-nu |k|^2 t) sin(omega t) / omega,  omega^2 = (k x b)(k x G) / |k|^2,
    k x b = kx by - ky bx; for omega^2 < 0 cosh and sinh of sqrt(-omega^2) t.  Returns (u, v, w, theta, amp_w, amp_theta, omega): the fields
    [nx, ny], the decayed (omega^2 > 0: the oscillation's envelope) or grown (omega^2 < 0) amplitudes of w and of theta's fluctuation, and
    omega (sqrt|omega^2|)."""
    kx, ky = 2 * np.pi * m[0] / Lx, 2 * np.pi * m[1] / Ly
    k2 = kx * kx + ky * ky
    kb, kg = kx * b[1] - ky * b[0], kx * G[1] - ky * G[0]
    w2 = kb * kg / k2
    om = np.sqrt(abs(w2))
    a0, dec = 1.0 / k2, np.exp(-nu * k2 * t)
    if w2 > 0:
        a, c = a0 * dec * np.cos(om * t), -kg * a0 * dec * np.sin(om * t) / om
        amp_w, amp_t = dec, abs(kg) * a0 * dec / om
    else:
        a, c = a0 * dec * np.cosh(om * t), -kg * a0 * dec * np.sinh(om * t) / om
        amp_w, amp_t = dec * np.cosh(om * t), abs(kg) * a0 * dec * np.sinh(om * t) / om
    X, Y = np.meshgrid(Lx * np.arange(nx) / nx, Ly * np.arange(ny) / ny, indexing='ij')
    phi = kx * (X - U[0] * t) + ky * (Y - U[1] * t)
    u = U[0] - a * ky * np.sin(phi)
    v = U[1] + a * kx * np.sin(phi)
    w = a * k2 * np.cos(phi)
    theta = c * np.sin(phi) - t * (G[0] * U[0] + G[1] * U[1])
    return u, v, w, theta, amp_w, amp_t, om
