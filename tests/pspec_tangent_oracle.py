"""NumPy float64 restatement (tests only) of the forward mode of the periodic solver's step (csrc/pspec_kernels.hip:
nns_spec_ns_step_tangent_f32; nns.periodic.PeriodicSolver.step_tangent / evolve_tangent): LinearScheme of tests/pspec_linear_oracle.py --
with nu_h = mu = beta = 0 the forced scheme of tests/pspec_forced_oracle.py, statement for statement -- plus its Jacobian-vector product.

The Lawson RK4 recurrences are linear in (w^, N^), so the tangent of a step is the same recurrence on (dw^, dN^) with the same factors
E = exp(lambda dt / 2), real or complex:

    d1 = E (dw + dt/2 dN0)       d2 = E dw + dt/2 dN1       d3 = E^2 dw + dt E dN2
    dw+ = E^2 (dw + dt/6 dN0) + dt/3 E (dN1 + dN2) + dt/6 dN3
    dN_i = N'(s_i) d_i + dg^ = -M [u d_x + v d_y + du w_x + dv w_y]^ + dg^

u, v, w_x, w_y those of the base's stage state s_i (the means (U0, V0) in u and v), du^ = i ky d^ / |k|^2, dv^ = -i kx d^ / |k|^2: the
perturbation has no mean flow (the mean is a constant of the call) and no (0, 0) mode, and takes the vorticity's mask.  The kick of a
stochastic step is additive and independent of the state: the base takes it (``starts``), the tangent does not.
"""
import numpy as np

import pspec_linear_oracle as LO

# deliberately wrong forward modes (mutation tests): du . grad w dropped; u . grad dw dropped; the mean flow missing from the tangent's
# advection; every stage linearised about s0 instead of s_i; the tangent product not dealiased; E^2 not applied to dw in stage 3
# (d3 = dw + dt E dN2); dg^ added in stage 1 only; conj(E), conj(E^2) on the tangent where E, E^2 belong (differs only in the linear form);
# the tangent's (0, 0) mode kept
WRONG = ('no_du_grad_w', 'no_u_grad_dw', 'no_mean_flow', 'frozen_base', 'not_dealiased', 'no_E_stage3', 'dg_one_stage', 'conj_E', 'keep_00')


class TangentScheme(LO.LinearScheme):
    """wrong: None, or one of WRONG.  The flow alone: no scalar (kappa = 0, no buoyancy)."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, hyper=(0.0, 2), hypo=(0.0, 1), beta=0.0, wrong=None):
        LO.LinearScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, hyper=hyper, hypo=hypo, beta=beta)
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.wrong = wrong

    def pair(self, a, b):
        """<a, b> per grid of two spectra of real fields: the grid sum of the product of the fields."""
        return (self.irfft2(a) * self.irfft2(b)).sum(axis=(-2, -1))

    def tangent_mask(self):
        if self.wrong in ('not_dealiased', 'keep_00'):
            m = np.ones_like(self.M) if self.wrong == 'not_dealiased' else self.M.copy()
            m[0, 0] = float(self.wrong == 'keep_00')
            return m
        return self.M

    def nonlinear_jvp(self, w, mean, dw):
        """N'(w) dw = -M [u dw_x + v dw_y + du w_x + dv w_y]^ (no source: step_jvp adds dg^)."""
        if self.wrong == 'no_mean_flow':
            mean = np.zeros_like(mean)
        uh, vh = self.velocity_hat(w, mean)
        u, v = self.irfft2(uh), self.irfft2(vh)
        wx, wy = self.irfft2(1j * self.kx * w), self.irfft2(1j * self.ky * w)
        duh, dvh = self.velocity_hat(dw, np.zeros_like(mean))
        du, dv = self.irfft2(duh), self.irfft2(dvh)
        dwx, dwy = self.irfft2(1j * self.kx * dw), self.irfft2(1j * self.ky * dw)
        prod = np.zeros_like(u)
        if self.wrong != 'no_u_grad_dw':
            prod = prod + u * dwx + v * dwy
        if self.wrong != 'no_du_grad_w':
            prod = prod + du * wx + dv * wy
        return -self.tangent_mask() * np.fft.rfft2(prod)

    def stages(self, w, mean):
        """(s0, s1, s2, s3) of one step from w: the statements of LinearScheme.step."""
        dt = self.dt
        E, E2 = self.factors()
        a = self.nonlinear(w, mean, 1)
        s1 = E * (w + dt / 2 * a)
        b = self.nonlinear(s1, mean, 2)
        s2 = E * w + dt / 2 * b
        c = self.nonlinear(s2, mean, 3)
        return w, s1, s2, E2 * w + dt * E * c

    def step_jvp(self, w, mean, dw, nsteps=1, dg=None, starts=None):
        """dw^ after nsteps steps: the Jacobian of those steps from w applied to dw^ (rfft2 layout [..., nx, nh]), plus the response to the
        source perturbation dg^ (constant over the call; leading axes broadcast).  starts: the start spectra of every step when they are not
        those of nsteps deterministic steps from w (a stochastic run: they carry the kicks); w and nsteps are then unused."""
        dt = self.dt
        E, E2 = self.factors()
        if self.wrong == 'conj_E':
            E, E2 = np.conj(E), np.conj(E2)
        Mt = self.tangent_mask()
        if starts is None:
            starts = []
            for _ in range(nsteps):
                starts.append(w)
                w = self.step(w, mean, 1)
        dw = Mt * np.asarray(dw, dtype=np.complex128)
        dg = np.zeros_like(dw) if dg is None else Mt * np.asarray(dg, dtype=np.complex128)
        for w0 in starts:
            s = self.stages(w0, mean)
            if self.wrong == 'frozen_base':
                s = (s[0],) * 4
            later = 0.0 if self.wrong == 'dg_one_stage' else dg
            da = self.nonlinear_jvp(s[0], mean, dw) + dg
            db = self.nonlinear_jvp(s[1], mean, E * (dw + dt / 2 * da)) + later
            dc = self.nonlinear_jvp(s[2], mean, E * dw + dt / 2 * db) + later
            d3 = (dw if self.wrong == 'no_E_stage3' else E2 * dw) + dt * E * dc
            dd = self.nonlinear_jvp(s[3], mean, d3) + later
            dw = E2 * dw + dt / 6 * (E2 * da + 2 * E * (db + dc) + dd)
        return dw
