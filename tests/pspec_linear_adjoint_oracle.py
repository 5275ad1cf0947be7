"""NumPy float64 restatement (tests only) of the reverse mode of the periodic solver's linear step, with or without its scalar, buoyancy and
white-in-time kick (csrc/pspec_kernels.hip: nns_spec_ns_step_linear_adjoint_f32; nns.periodic.PeriodicSolver.evolve / evolve_velocity):
LinearScheme of tests/pspec_linear_oracle.py plus its vector-Jacobian product, for the flow and for the system (w^, theta^).

Cotangents are real band-limited fields paired by the plain grid sum <a, b> = sum a b and kept as their rfft2 spectra, as in
tests/pspec_adjoint_oracle.py and tests/pspec_scalar_adjoint_oracle.py, whose N'(s)^T this file takes unchanged (beta sits in lambda, not in
N).  The Lawson factor E_k = exp(lambda_k dt / 2) is complex with E(-k) = conj(E(k)), so z -> E z maps spectra of real fields to such, and

    <a, E b> = (1 / n) sum_k Re(conj(a_k) E_k b_k) = (1 / n) sum_k Re(conj(conj(E_k) a_k) b_k) = <conj(E) a, b>:

the transpose of E is multiplication by conj(E).  The recurrences of the two parents hold with F = conj(E), F2 = conj(E^2) on
(lam, kappa, r_w, wbar) and the real E_theta on (mu, m, r_theta, thetabar):

    k4 = dt/6 lam                    (r_w, r_theta) at s3    wbar  = F2 (lam + r_w)
    k3 = dt/3 F lam + dt F r_w       at s2                   wbar += F r_w
    k2 = dt/3 F lam + dt/2 r_w       at s1                   wbar += F r_w
    k1 = dt/6 F2 lam + dt/2 F r_w    at s0                   wbar += r_w
    gbar = k1 + k2 + k3 + k4

The kick of a stochastic step, w^ += sqrt(dt) a xi after the complete step, is additive and independent of the state: its Jacobian in w^ is the
identity.  The reverse mode of a stochastic run is therefore the deterministic step's, linearised about the stage states of the NOISY trajectory:
step_vjp takes the start spectra of every step (``starts``), which carry the kicks (stochastic_vjp).
"""
import numpy as np

import pspec_linear_oracle as LO
import pspec_scalar_adjoint_oracle as SA
import pspec_stochastic_oracle as ST

# deliberately wrong reverse modes (mutation tests): E where conj(E) belongs; |E|, the rotation forgotten; conj(E^2) rotated by the angle of E
# instead of twice it; the real factors exp(-(nu |k|^2 + drag) dt / 2) of the steady adjoint, the table ignored; the stage states shifted by
# one (s0, s0, s1, s2 where s0, s1, s2, s3 belong)
WRONG = ('not_conjugated', 'modulus_only', 'E2_angle_of_E', 'table_ignored', 'stage_shift')
# and of a stochastic run: the stage states recomputed from a kick-free trajectory
WRONG_STOCHASTIC = ('kicks_dropped',)


class LinearAdjointScheme(LO.LinearScheme):
    """wrong: None, or one of WRONG.  Without a scalar build it with kappa = 0, grad = buoy = (0, 0) and leave t, mu out."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, kappa=0.0, grad=(0.0, 0.0), buoy=(0.0, 0.0),
                 hyper=(0.0, 2), hypo=(0.0, 1), beta=0.0, wrong=None):
        LO.LinearScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, kappa=kappa, grad=grad, buoy=buoy, hyper=hyper, hypo=hypo, beta=beta)
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.wrong = wrong

    # N'(s)^T, the pairing and the ends of evolve_velocity are the scalar adjoint's (with t = 0 and m = 0 the flow's)
    rfft2 = SA.ScalarAdjointScheme.rfft2
    pair = SA.ScalarAdjointScheme.pair
    nonlinear_vjp = SA.ScalarAdjointScheme.nonlinear_vjp
    velocity = SA.ScalarAdjointScheme.velocity
    velocity_vjp = SA.ScalarAdjointScheme.velocity_vjp
    init_vjp = SA.ScalarAdjointScheme.init_vjp

    def scalar_factors(self):
        lt = self.kappa * self.k2
        return np.exp(-lt * self.dt / 2), np.exp(-lt * self.dt)

    def adjoint_factors(self):
        """(F, F2): the transposes of the forward's E, E^2 -- their conjugates."""
        E, E2 = self.factors()
        if self.wrong == 'not_conjugated':
            return E, E2
        if self.wrong == 'modulus_only':
            return np.abs(E), np.abs(E2)
        if self.wrong == 'table_ignored':
            rate = self.nu * self.k2 + self.drag
            return np.exp(-rate * self.dt / 2), np.exp(-rate * self.dt)
        if self.wrong == 'E2_angle_of_E':
            return np.conj(E), np.abs(E2) * np.exp(-1j * np.angle(E))
        return np.conj(E), np.conj(E2)

    def stages(self, w, mean, t=None):
        """(s0, s1, s2, s3) of one step from w, or with t ((w, t) of s0, s1, s2, s3): the statements of LinearScheme.step."""
        dt = self.dt
        E, E2 = self.factors()
        if t is None:
            a = self.nonlinear(w, mean, 1)
            s1 = E * (w + dt / 2 * a)
            b = self.nonlinear(s1, mean, 2)
            s2 = E * w + dt / 2 * b
            c = self.nonlinear(s2, mean, 3)
            return w, s1, s2, E2 * w + dt * E * c
        Et, Et2 = self.scalar_factors()
        a, at = self.nonlinear_w(w, t, mean, 1), self.nonlinear_scalar(w, t, mean)
        w2, t2 = E * (w + dt / 2 * a), Et * (t + dt / 2 * at)
        b, bt = self.nonlinear_w(w2, t2, mean, 2), self.nonlinear_scalar(w2, t2, mean)
        w3, t3 = E * w + dt / 2 * b, Et * t + dt / 2 * bt
        c, ct = self.nonlinear_w(w3, t3, mean, 3), self.nonlinear_scalar(w3, t3, mean)
        return (w, t), (w2, t2), (w3, t3), (E2 * w + dt * E * c, Et2 * t + dt * Et * ct)

    def step_vjp(self, w, mean, lam, nsteps=1, t=None, mu=None, starts=None):
        """(wbar, gbar), or with a scalar (t, mu) (wbar, thetabar, gbar): the cotangents of the start spectra and of the vorticity source g^ (one
        per grid, summed over the steps) for the cotangents of the spectra after nsteps steps from w (and t).  starts: the start spectra of every
        step, w or (w, t) each, when they are not those of nsteps deterministic steps from w (a stochastic run); w, t and nsteps are then unused."""
        dt = self.dt
        scalar = t is not None
        F, F2 = self.adjoint_factors()
        Et, Et2 = self.scalar_factors()
        if starts is None:
            starts = []
            for _ in range(nsteps):
                starts.append((w, t) if scalar else w)
                if scalar:
                    w, t = self.step(w, t, mean, 1)
                else:
                    w = self.step(w, mean, 1)
        lam = self.M * np.asarray(lam, dtype=np.complex128)
        mu = self.Mt * np.asarray(mu, dtype=np.complex128) if scalar else np.zeros_like(lam)
        gbar = np.zeros_like(lam)
        zero = np.zeros_like(lam)
        for s in reversed(starts):
            st = self.stages(s[0], mean, s[1]) if scalar else [(x, zero) for x in self.stages(s, mean)]
            if self.wrong == 'stage_shift':
                st = [st[0], st[0], st[1], st[2]]
            s0, s1, s2, s3 = st
            k4, m4 = dt / 6 * lam, dt / 6 * mu
            rw, rt = self.nonlinear_vjp(s3[0], s3[1], mean, k4, m4)
            wbar, tbar = F2 * (lam + rw), Et2 * (mu + rt)
            k3, m3 = dt / 3 * F * lam + dt * F * rw, dt / 3 * Et * mu + dt * Et * rt
            rw, rt = self.nonlinear_vjp(s2[0], s2[1], mean, k3, m3)
            wbar, tbar = wbar + F * rw, tbar + Et * rt
            k2, m2 = dt / 3 * F * lam + dt / 2 * rw, dt / 3 * Et * mu + dt / 2 * rt
            rw, rt = self.nonlinear_vjp(s1[0], s1[1], mean, k2, m2)
            wbar, tbar = wbar + F * rw, tbar + Et * rt
            k1, m1 = dt / 6 * F2 * lam + dt / 2 * F * rw, dt / 6 * Et2 * mu + dt / 2 * Et * rt
            rw, rt = self.nonlinear_vjp(s0[0], s0[1], mean, k1, m1)
            wbar, tbar = wbar + rw, tbar + rt
            gbar = gbar + k1 + k2 + k3 + k4
            lam, mu = wbar, tbar
        return (lam, mu, gbar) if scalar else (lam, gbar)


def stochastic_starts(S, amp, seed, w, mean, nsteps, t=None, ids=None, n0=0):
    """(starts, w[, t]): the start spectra of every step of the stochastic run (pspec_stochastic_oracle.Stochastic on S) and its end state."""
    X = ST.Stochastic(S, amp, seed)
    starts = []
    for n in range(n0, n0 + nsteps):
        starts.append(w if t is None else (w, t))
        if t is None:
            w = X.step(w, mean, 1, ids=ids, n0=n)
        else:
            w, t = X.step(w, mean, 1, t=t, ids=ids, n0=n)
    return (starts, w) if t is None else (starts, w, t)


def stochastic_vjp(S, amp, seed, w, mean, lam, nsteps, t=None, mu=None, ids=None, n0=0, wrong=None):
    """step_vjp of the stochastic run: the deterministic step's reverse mode about the noisy trajectory.  wrong = 'kicks_dropped': about the
    kick-free trajectory from the same start."""
    if wrong is not None and wrong not in WRONG_STOCHASTIC:
        raise ValueError(wrong)
    if wrong == 'kicks_dropped':
        return S.step_vjp(w, mean, lam, nsteps, t=t, mu=mu)
    starts = stochastic_starts(S, amp, seed, w, mean, nsteps, t=t, ids=ids, n0=n0)[0]
    return S.step_vjp(w, mean, lam, nsteps, t=t, mu=mu, starts=starts)
