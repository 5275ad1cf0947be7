"""NumPy float64 restatement (tests only) of the forward mode of the periodic solver's step with a scalar (csrc/pspec_kernels.hip:
nns_spec_ns_step_scalar_tangent_f32; nns.periodic.PeriodicSolver.step_tangent_scalar / evolve_tangent_scalar): LinearAdjointScheme of
tests/pspec_linear_adjoint_oracle.py -- LinearScheme with its stage states and its vector-Jacobian product -- plus the Jacobian-vector
product of the system (w^, theta^).

The Lawson RK4 recurrences are linear in (w^, N_w^) and in (theta^, N_theta^), so the tangent of a step is the same recurrence on
(dw^, dtheta^), dw^ with the vorticity's factors E = exp(lambda dt / 2) (real or complex) and dtheta^ with the scalar's real E_theta:

    d1 = E (d + dt/2 dN0)       d2 = E d + dt/2 dN1       d3 = E^2 d + dt E dN2
    d+ = E^2 (d + dt/6 dN0) + dt/3 E (dN1 + dN2) + dt/6 dN3

    dN_w     = -M       [u dw_x + v dw_y + du w_x + dv w_y]^ + dg^ + M (i kx by - i ky bx) dtheta^
    dN_theta = -M_theta [u dtheta_x + v dtheta_y + du (theta_x + Gx) + dv (theta_y + Gy)]^

about every stage's own state s_i = (w, theta)_i: u, v those of s_i with the means (U0, V0), du^ = i ky dw^ / |k|^2, dv^ = -i kx dw^ / |k|^2.
The perturbation has no mean flow; dw^ has no (0, 0) mode; dtheta^ takes M_theta, which keeps (0, 0): its mean is carried unchanged (the
(0, 0) mode of a product u . grad f of a divergence-free u with a periodic f vanishes, and du has no mean to meet G) and acts on nothing.
The scalar has no source and takes no kick; a stochastic base takes its kicks (``starts``), the tangent none.  With b = (0, 0) the dw^ half
is TangentScheme.step_jvp of tests/pspec_tangent_oracle.py.
"""
import numpy as np

import pspec_linear_adjoint_oracle as LA

# deliberately wrong forward modes (mutation tests): du . (grad theta + G) dropped from dN_theta; the mean gradient G missing there; the
# buoyancy of dtheta missing from dN_w; its sign flipped; dtheta^ under the vorticity's mask (its mean dropped); the vorticity's E, E^2 on
# dtheta^ where E_theta belongs; theta of every stage frozen at the step's start (the flow's stages right); every stage linearised about
# s0; the tangent products not dealiased
WRONG = ('no_du_grad_theta', 'no_G', 'no_dbuoy', 'buoy_sign', 'theta_drops_00', 'E_on_theta', 'frozen_theta', 'frozen_base', 'not_dealiased')


class ScalarTangentScheme(LA.LinearAdjointScheme):
    """wrong: None, or one of WRONG (this file's; the adjoint half stays right)."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, drag=0.0, kappa=0.0, grad=(0.0, 0.0), buoy=(0.0, 0.0),
                 hyper=(0.0, 2), hypo=(0.0, 1), beta=0.0, wrong=None):
        LA.LinearAdjointScheme.__init__(self, nx, ny, dt, rho, nu, Lx, Ly, drag=drag, kappa=kappa, grad=grad, buoy=buoy, hyper=hyper, hypo=hypo,
                                        beta=beta)
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.twrong = wrong

    def tangent_masks(self):
        """(the mask of dN_w, the mask of dN_theta)."""
        if self.twrong == 'not_dealiased':
            mw, mt = np.ones_like(self.M), np.ones_like(self.M)
            mw[0, 0] = 0.0
            return mw, mt
        return self.M, (self.M if self.twrong == 'theta_drops_00' else self.Mt)

    def nonlinear_jvp(self, w, t, mean, dw, dt):
        """(dN_w, dN_theta) = N'(w, theta) (dw, dtheta), without dg^ (step_jvp adds it)."""
        mw, mt = self.tangent_masks()
        uh, vh = self.velocity_hat(w, mean)
        u, v = self.irfft2(uh), self.irfft2(vh)
        wx, wy = self.irfft2(1j * self.kx * w), self.irfft2(1j * self.ky * w)
        tx, ty = self.irfft2(1j * self.kx * t), self.irfft2(1j * self.ky * t)
        duh, dvh = self.velocity_hat(dw, np.zeros_like(mean))
        du, dv = self.irfft2(duh), self.irfft2(dvh)
        dwx, dwy = self.irfft2(1j * self.kx * dw), self.irfft2(1j * self.ky * dw)
        dtx, dty = self.irfft2(1j * self.kx * dt), self.irfft2(1j * self.ky * dt)
        gx, gy = (0.0, 0.0) if self.twrong == 'no_G' else self.grad
        nw = -mw * np.fft.rfft2(u * dwx + v * dwy + du * wx + dv * wy)
        bx, by = self.buoy
        if self.twrong == 'buoy_sign':
            bx, by = -bx, -by
        if self.twrong != 'no_dbuoy' and (bx, by) != (0.0, 0.0):
            nw = nw + mw * (1j * self.kx * by - 1j * self.ky * bx) * dt
        prod = u * dtx + v * dty
        if self.twrong != 'no_du_grad_theta':
            prod = prod + du * (tx + gx) + dv * (ty + gy)
        return nw, -mt * np.fft.rfft2(prod)

    def step_jvp(self, w, t, mean, dw, dtheta, nsteps=1, dg=None, starts=None):
        """(dw^, dtheta^) after nsteps steps: the Jacobian of those steps from (w, t) applied to the pair (rfft2 layout [..., nx, nh]), plus the
        response to the vorticity source's perturbation dg^ (constant over the call).  starts: the start spectra (w, t) of every step when they
        are not those of nsteps deterministic steps from (w, t) (a stochastic run: they carry the kicks); w, t and nsteps are then unused."""
        h = self.dt
        E, E2 = self.factors()
        Et, Et2 = (E, E2) if self.twrong == 'E_on_theta' else self.scalar_factors()
        mw, mt = self.tangent_masks()
        if starts is None:
            starts = []
            for _ in range(nsteps):
                starts.append((w, t))
                w, t = self.step(w, t, mean, 1)
        dw = mw * np.asarray(dw, dtype=np.complex128)
        dq = mt * np.asarray(dtheta, dtype=np.complex128)
        dg = np.zeros_like(dw) if dg is None else mw * np.asarray(dg, dtype=np.complex128)
        for w0, t0 in starts:
            s = self.stages(w0, mean, t0)
            if self.twrong == 'frozen_base':
                s = (s[0],) * 4
            elif self.twrong == 'frozen_theta':
                s = tuple((x[0], s[0][1]) for x in s)
            a, at = self.nonlinear_jvp(s[0][0], s[0][1], mean, dw, dq)
            a = a + dg
            b, bt = self.nonlinear_jvp(s[1][0], s[1][1], mean, E * (dw + h / 2 * a), Et * (dq + h / 2 * at))
            b = b + dg
            c, ct = self.nonlinear_jvp(s[2][0], s[2][1], mean, E * dw + h / 2 * b, Et * dq + h / 2 * bt)
            c = c + dg
            d, dth = self.nonlinear_jvp(s[3][0], s[3][1], mean, E2 * dw + h * E * c, Et2 * dq + h * Et * ct)
            d = d + dg
            dw = E2 * dw + h / 6 * (E2 * a + 2 * E * (b + c) + d)
            dq = Et2 * dq + h / 6 * (Et2 * at + 2 * Et * (bt + ct) + dth)
        return dw, dq
