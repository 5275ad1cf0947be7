"""NumPy float64 restatement (tests only) of the second-order adjoint of the periodic solver's step (csrc/pspec_kernels.hip:
nns_spec_ns_step_second_adjoint_f32; nns.periodic.PeriodicSolver.second_order_forward / hessian_vector_product): the reverse mode of
tests/pspec_linear_adjoint_oracle.py (LinearAdjointScheme.step_vjp, the flow alone) differentiated in a direction (dw, dg, dlam), with the
tangent stages of tests/pspec_tangent_oracle.py (TangentScheme.step_jvp).

step_vjp is (w, g, lam) -> (wbar, gbar).  Its derivative in (dw, dg, dlam): the stage states s_i move by the tangent stages d_i, the
cotangents lam, k_i, r by dlam, dk_i, dr.  The nonlinear term is bilinear, so

    N'(s)^T k = M [u k_x + v k_y]^ - M [k_x w_y - k_y w_x]^ / |k|^2        (u, v, w_x, w_y of s, the means in u, v)

is linear in k and affine in s, and its derivative is N'(s)^T dk + N'_0(d)^T k, N'_0 the same expression with u, v, w_x, w_y of d and zero
mean flow (the mean is a constant of the call).  The Lawson recurrences are linear with constant factors F = conj(E), F2 = conj(E^2), so

    k4 = dt/6 lam                  dk4 = dt/6 dlam
    r  = N'(s3)^T k4               dr  = N'(s3)^T dk4 + N'_0(d3)^T k4      wbar  = F2 (lam + r)    dwbar  = F2 (dlam + dr)
    k3 = dt/3 F lam + dt F r       dk3 = dt/3 F dlam + dt F dr
    r  = N'(s2)^T k3               dr  = N'(s2)^T dk3 + N'_0(d2)^T k3      wbar += F r             dwbar += F dr
    k2 = dt/3 F lam + dt/2 r       dk2 = dt/3 F dlam + dt/2 dr
    r  = N'(s1)^T k2               dr  = N'(s1)^T dk2 + N'_0(d1)^T k2      wbar += F r             dwbar += F dr
    k1 = dt/6 F2 lam + dt/2 F r    dk1 = dt/6 F2 dlam + dt/2 F dr
    r  = N'(s0)^T k1               dr  = N'(s0)^T dk1 + N'_0(d0)^T k1      wbar += r               dwbar += dr
    gbar += k1 + k2 + k3 + k4      dgbar += dk1 + dk2 + dk3 + dk4

The left column is step_vjp's, statement for statement, and the tangent stages are step_jvp's: the first-order results are the parents' to
the last bit.  A stochastic step is differentiated as the deterministic step it contains (``starts`` carry the kicks; the tangent takes none).

With l = 1/2 sum (w_N - obs)^2, lam = w_N - obs and dlam = dw_N, (dwbar, dgbar) is the Hessian of l applied to (dw, dg), symmetric jointly
in (w, g); dlam = 0 leaves the part a Gauss-Newton product drops, sum lam . d^2 Phi[d, .].
"""
import numpy as np

import pspec_linear_adjoint_oracle as LA
import pspec_tangent_oracle as T

# deliberately wrong second-order adjoints (mutation tests): N'_0(d)^T k dropped (the Gauss-Newton product); the mean flow left in the
# tangent stage's velocity; every stage's tangent taken as d0; the tangent stages shifted by one (d0, d0, d1, d2 where d0, d1, d2, d3
# belong); the tangent stage's velocity without its inverse Laplacian (du^ = i ky d^); E, E^2 where conj(E), conj(E^2) belong, on the second
# quadruple only (differs only in the linear form)
WRONG = ('gauss_newton', 'mean_in_du', 'frozen_tangent', 'stage_shift_d', 'no_ilap_d', 'not_conjugated')


class SecondAdjointScheme(LA.LinearAdjointScheme, T.TangentScheme):
    """wrong: None, or one of WRONG; the parents' own mutations stay off.  The flow alone: no scalar."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, hyper=(0.0, 2), hypo=(0.0, 1), beta=0.0, wrong=None):
        LA.LinearAdjointScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, hyper=hyper, hypo=hypo, beta=beta)
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.wrong2 = wrong

    pair = LA.LinearAdjointScheme.pair

    def stages(self, w, mean):
        return T.TangentScheme.stages(self, w, mean)

    def state_vjp(self, s, mean, k):
        """N'(s)^T k: the parents' (the flow's share of the scalar adjoint's, t = 0 and m = 0)."""
        zero = np.zeros_like(k)
        return self.nonlinear_vjp(s, zero, mean, k, zero)[0]

    def tangent_vjp(self, d, mean, k):
        """N'_0(d)^T k = M [du k_x + dv k_y]^ - M [k_x d_y - k_y d_x]^ / |k|^2, du^ = i ky d^ / |k|^2, dv^ = -i kx d^ / |k|^2: no mean flow."""
        if self.wrong2 == 'gauss_newton':
            return np.zeros_like(k)
        k = self.M * k
        m = mean if self.wrong2 == 'mean_in_du' else np.zeros_like(mean)
        uh, vh = self.velocity_hat(d * self.k2 if self.wrong2 == 'no_ilap_d' else d, m)
        u, v = self.irfft2(uh), self.irfft2(vh)
        dx, dy = self.irfft2(1j * self.kx * d), self.irfft2(1j * self.ky * d)
        kx_, ky_ = self.irfft2(1j * self.kx * k), self.irfft2(1j * self.ky * k)
        return self.M * (np.fft.rfft2(u * kx_ + v * ky_) - np.fft.rfft2(kx_ * dy - ky_ * dx) * self.ik2)

    def step_second_vjp(self, w, mean, dw, dg, lam, dlam, nsteps=1, starts=None):
        """(wbar, gbar, dwbar, dgbar, dw_end): step_vjp's (wbar, gbar) for the cotangent lam of the spectrum after nsteps steps from w, their
        derivatives in the direction (dw, dg, dlam) -- dw the perturbation of the start spectrum, dg that of the source (None: none; constant
        over the call), dlam that of lam (None: zero) -- and step_jvp's dw after the steps.  All rfft2 layout [..., nx, nh].  starts: the start
        spectra of every step when they are not those of nsteps deterministic steps from w (a stochastic run); w and nsteps are then unused."""
        dt = self.dt
        E, E2 = self.factors()
        F, F2 = self.adjoint_factors()
        G, G2 = (E, E2) if self.wrong2 == 'not_conjugated' else (F, F2)            # the second quadruple's factors
        if starts is None:
            starts = []
            for _ in range(nsteps):
                starts.append(w)
                w = self.step(w, mean, 1)
        dw = self.M * np.asarray(dw, dtype=np.complex128)
        dg = np.zeros_like(dw) if dg is None else self.M * np.asarray(dg, dtype=np.complex128)
        steps = []
        for w0 in starts:                                                          # the tangent forward: step_jvp's statements, the stages kept
            s = self.stages(w0, mean)
            da = self.nonlinear_jvp(s[0], mean, dw) + dg
            d1 = E * (dw + dt / 2 * da)
            db = self.nonlinear_jvp(s[1], mean, d1) + dg
            d2 = E * dw + dt / 2 * db
            dc = self.nonlinear_jvp(s[2], mean, d2) + dg
            d3 = E2 * dw + dt * E * dc
            dd = self.nonlinear_jvp(s[3], mean, d3) + dg
            steps.append((s, (dw, d1, d2, d3)))
            dw = E2 * dw + dt / 6 * (E2 * da + 2 * E * (db + dc) + dd)
        lam = self.M * np.asarray(lam, dtype=np.complex128)
        dlam = np.zeros_like(lam) if dlam is None else self.M * np.asarray(dlam, dtype=np.complex128)
        gbar, dgbar = np.zeros_like(lam), np.zeros_like(lam)
        for s, d in reversed(steps):
            if self.wrong2 == 'frozen_tangent':
                d = (d[0],) * 4
            elif self.wrong2 == 'stage_shift_d':
                d = (d[0], d[0], d[1], d[2])
            k4, dk4 = dt / 6 * lam, dt / 6 * dlam
            rw, dr = self.state_vjp(s[3], mean, k4), self.state_vjp(s[3], mean, dk4) + self.tangent_vjp(d[3], mean, k4)
            wbar, dwbar = F2 * (lam + rw), G2 * (dlam + dr)
            k3, dk3 = dt / 3 * F * lam + dt * F * rw, dt / 3 * G * dlam + dt * G * dr
            rw, dr = self.state_vjp(s[2], mean, k3), self.state_vjp(s[2], mean, dk3) + self.tangent_vjp(d[2], mean, k3)
            wbar, dwbar = wbar + F * rw, dwbar + G * dr
            k2, dk2 = dt / 3 * F * lam + dt / 2 * rw, dt / 3 * G * dlam + dt / 2 * dr
            rw, dr = self.state_vjp(s[1], mean, k2), self.state_vjp(s[1], mean, dk2) + self.tangent_vjp(d[1], mean, k2)
            wbar, dwbar = wbar + F * rw, dwbar + G * dr
            k1, dk1 = dt / 6 * F2 * lam + dt / 2 * F * rw, dt / 6 * G2 * dlam + dt / 2 * G * dr
            rw, dr = self.state_vjp(s[0], mean, k1), self.state_vjp(s[0], mean, dk1) + self.tangent_vjp(d[0], mean, k1)
            wbar, dwbar = wbar + rw, dwbar + dr
            gbar, dgbar = gbar + k1 + k2 + k3 + k4, dgbar + dk1 + dk2 + dk3 + dk4
            lam, dlam = wbar, dwbar
        return lam, gbar, dlam, dgbar, dw
