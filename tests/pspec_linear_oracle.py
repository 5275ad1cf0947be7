"""NumPy float64 restatement (tests only) of the general linear operator of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_linear_f32, nns_spec_ns_linear_spectrum_f32; nns.periodic.PeriodicSolver with hyperviscosity, hypofriction and beta):
tests/pspec_buoyant_oracle.py (and with it the forced and the scalar scheme) plus hyperviscosity, hypofriction and the beta effect,

    w_t + u w_x + v w_y + beta v' = nu lap w - nu_h (-lap)^p w - alpha w - mu (-lap)^-q w + g + (by theta_x - bx theta_y)

v' = v - <v>: beta <v> would be a constant source in the (0, 0) mode, which the periodic box cannot hold, so it is dropped and the mean velocity
stays conserved.  With psi^ = w^ / |k|^2 and v^ = -i kx psi^ the linear part of mode k is

    lambda_k = -(nu |k|^2 + alpha + nu_h |k|^2p + mu |k|^-2q) + i beta kx / |k|^2,          lambda_(0,0) = 0

Lawson RK4 as in the parents with the complex E = exp(lambda dt / 2), E^2 = exp(lambda dt); N keeps its definition (force, buoyancy, every
stage's own velocity), the scalar its operator -kappa |k|^2.  Re(lambda) is even in k and Im(lambda) odd, so the field stays real.  A single
plane wave is an exact nonlinear solution: frequency omega = -beta kx / |k|^2 (westward), amplitude exp(Re(lambda) t) (rossby_wave).
Rates: d/dt 1/2 |w^|^2 = Re(lambda) |w^|^2 + (nonlinear, force), so per shell (tests/pspec_spectrum_oracle.py)
    D_E(s) = sum wt Re(lambda_k) |w^_k|^2 / |k|^2 / n^2,   D_Z(s) = sum wt Re(lambda_k) |w^_k|^2 / n^2,   dE(s)/dt = T_E + F + D_E (+ B);
beta contributes to neither.
"""
import numpy as np

import pspec_buoyant_oracle as BO
import pspec_spectrum_oracle as PO

# deliberately wrong schemes (mutation tests): 'sign': -beta; 'ky': beta ky / |k|^2 instead of kx; 'conj': conj E and conj E^2; 'order': the
# hyperviscosity of order p - 1; 'nohypo': no hypofriction; 'realE2': E^2 rotated by the angle of E instead of twice it
MUTATIONS = ('sign', 'ky', 'conj', 'order', 'nohypo', 'realE2')


class LinearScheme(BO.BuoyantScheme):
    """hyper = (nu_h, p), hypo = (mu, q), beta; mutate: one of MUTATIONS.  ``step`` takes (w, mean[, nsteps]) for the flow alone and
    (w, t, mean[, nsteps]) with a scalar, so tests/pspec_stochastic_oracle.py: Stochastic can drive it either way."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, kappa=0.0, grad=(0.0, 0.0), buoy=(0.0, 0.0),
                 hyper=(0.0, 2), hypo=(0.0, 1), beta=0.0, mutate=None):
        BO.BuoyantScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, kappa=kappa, grad=grad, buoy=buoy)
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError("mutate must be None or one of %s" % (MUTATIONS,))
        self.hyper, self.hypo, self.beta, self.lmutate = (float(hyper[0]), int(hyper[1])), (float(hypo[0]), int(hypo[1])), float(beta), mutate

    def damping(self):
        """-Re(lambda) [nx, nh] >= 0 on every mode but (0, 0) (0 there when a hypofriction is present; the mask keeps that mode out anyway).
        With nu_h = mu = 0 the expression of the parents, nu |k|^2 + alpha."""
        lam = self.nu * self.k2 + self.drag
        (nu_h, p), (mu, q) = self.hyper, self.hypo
        if nu_h > 0:
            lam = lam + nu_h * self.k2 ** (p - 1 if self.lmutate == 'order' else p)
        if mu > 0 and self.lmutate != 'nohypo':
            lam = lam + mu * self.ik2 ** q
        return lam

    def rotation(self):
        """Im(lambda) [nx, nh] = beta kx / |k|^2 (0 at (0, 0)), or None with beta = 0."""
        if self.beta == 0.0:
            return None
        beta = -self.beta if self.lmutate == 'sign' else self.beta
        return beta * (self.ky if self.lmutate == 'ky' else self.kx) * self.ik2

    def linear_operator(self):
        """lambda [nx, nh] (complex128) on the kept modes, 0 elsewhere and at (0, 0); compact() gives the solver's layout."""
        rot = self.rotation()
        return self.M * (-self.damping() + 1j * (0.0 if rot is None else rot))

    def factors(self):
        """(E, E^2): real arrays with beta = 0 (the parents' statements), complex otherwise."""
        dt, lam, rot = self.dt, self.damping(), self.rotation()
        E = np.exp(-lam * dt / 2)
        E2 = np.exp(-lam * dt)
        if rot is not None:
            ph = np.exp(1j * rot * dt / 2)
            E, E2 = E * ph, E2 * (ph if self.lmutate == 'realE2' else ph * ph)
            if self.lmutate == 'conj':
                E, E2 = np.conj(E), np.conj(E2)
        return E, E2

    def step(self, w, *args, **kw):
        if len(args) >= 2 and not np.isscalar(args[1]):
            (t, mean), rest = args[:2], args[2:]
        else:
            t, mean, rest = None, args[0], args[1:]
        nsteps = rest[0] if rest else kw.get('nsteps', 1)
        dt = self.dt
        E, E2 = self.factors()
        if t is None:
            for _ in range(nsteps):
                a = self.nonlinear(w, mean, 1)
                b = self.nonlinear(E * (w + dt / 2 * a), mean, 2)
                c = self.nonlinear(E * w + dt / 2 * b, mean, 3)
                d = self.nonlinear(E2 * w + dt * E * c, mean, 4)
                w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
            return w
        lt = self.kappa * self.k2
        Et = np.exp(-lt * dt / 2)
        Et2 = np.exp(-lt * dt)
        for _ in range(nsteps):
            a = self.nonlinear_w(w, t, mean, 1)
            at = self.nonlinear_scalar(w, t, mean)
            w2, t2 = E * (w + dt / 2 * a), Et * (t + dt / 2 * at)
            b = self.nonlinear_w(w2, t2, mean, 2)
            bt = self.nonlinear_scalar(w2, t2, mean)
            w3, t3 = E * w + dt / 2 * b, Et * t + dt / 2 * bt
            c = self.nonlinear_w(w3, t3, mean, 3)
            ct = self.nonlinear_scalar(w3, t3, mean)
            w4, t4 = E2 * w + dt * E * c, Et2 * t + dt * Et * ct
            d = self.nonlinear_w(w4, t4, mean, 4)
            dth = self.nonlinear_scalar(w4, t4, mean)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
            t = Et2 * t + dt / 6 * (Et2 * at + 2 * Et * (bt + ct) + dth)
        return w, t

    def linear_modes(self, w):
        """Re(lambda_k) |w^_k|^2 per mode."""
        return self.linear_operator().real * (w.real ** 2 + w.imag ** 2)

    def linear_spectrum(self, w):
        """(D_E, D_Z), each [..., S]: the linear term's energy and enstrophy rates by the shells of tests/pspec_spectrum_oracle.py."""
        m = self.linear_modes(w)
        return PO.bin_shells(self, m * self.ik2), PO.bin_shells(self, m)

    def energy_budget(self, w, t=None):
        """dE(s)/dt = T_E + F + D_E (+ B with a scalar), [..., S]."""
        rhs = PO.transfer(self, w)['T_E'] + PO.spectrum(self, w)['F'] + self.linear_spectrum(w)[0]
        return rhs if t is None else rhs + self.buoyancy_spectrum(w, t)


def rossby_wave(nx, ny, t, m, beta, damping, U=(0.0, 0.0), Lx=2 * np.pi, Ly=2 * np.pi):
    """The exact solution for a single wavevector k = 2 pi (m_x / Lx, m_y / Ly) on the mean flow U = (U0, V0), vorticity amplitude 1 at t = 0:
        w = A cos phi,   phi = k . (x - U t) - omega t,   omega = -beta kx / |k|^2,   A = exp(-damping t),   damping = -Re(lambda_k)
    (the nonlinear term vanishes identically; beta acts on v' = v - V0 only).  Returns (u, v, w, A, omega): the fields [nx, ny]; p = 0."""
    kx, ky = 2 * np.pi * m[0] / Lx, 2 * np.pi * m[1] / Ly
    k2 = kx * kx + ky * ky
    om = -beta * kx / k2
    A = np.exp(-damping * t)
    X, Y = np.meshgrid(Lx * np.arange(nx) / nx, Ly * np.arange(ny) / ny, indexing='ij')
    phi = kx * (X - U[0] * t) + ky * (Y - U[1] * t) - om * t
    a = A / k2
    return U[0] - a * ky * np.sin(phi), U[1] + a * kx * np.sin(phi), A * np.cos(phi), A, om
