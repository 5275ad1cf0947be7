"""NumPy float64 restatement (tests only) of the periodic solver's reverse mode in its LINEAR OPERATOR (csrc/pspec_kernels.hip:
nns_spec_ns_step_operator_adjoint_f32; nns.periodic.PeriodicSolver.evolve / evolve_velocity with ``operator``, ``operator_table``):
LinearAdjointScheme of tests/pspec_linear_adjoint_oracle.py, its factors read from a table l = lambda dt / 2 per mode that can be perturbed,
plus the vector-Jacobian product in that table, for the flow, the scalar, the buoyant and the stochastic step.

With E = exp(l) the Lawson RK4 step

    s1 = E (w0 + dt/2 N0)      s2 = E w0 + dt/2 N1      s3 = E^2 w0 + dt E N2      w1 = E^2 w0 + dt/6 (E^2 N0 + 2 E N1 + 2 E N2 + N3)

depends on l per mode, directly, through (no N, no division by E)

    d s1 / dl = s1      d s2 / dl = E w0      d s3 / dl = s3 + E^2 w0      d w1 / dl = (s3 + E^2 w0) / 3 + 2/3 E (s1 + s2)

and a cotangent c of z = D dl pairs as Re(conj(c) D dl) = Re(c conj(D)) dRe l + Im(c conj(D)) dIm l.  The cotangent of w1 is lam, that of s_S is
r_S = N'(s_S)^T k_(S+1), which the recurrences of the parent file already form, so one step adds per mode

    T += (r3 + lam / 3) conj(s3 + E^2 w0) + r2 conj(E w0) + 2/3 lam conj(E s2) + (r1 + 2/3 conj(E) lam) conj(s1).

Cotangents are spectra (unnormalised rfft2) of real fields paired by the plain grid sum, <a, b> = (1 / n) sum over the FULL spectrum of
Re(conj(a_k) b_k), n = nx ny.  A table obeys l(-k) = conj(l(k)); its stored entries are those of the solver's layout: every kx for ky >= 0.
A stored mode with ky > 0 stands for itself and its mirror image, which contribute equally: weight 2 / n.  On the ky = 0 line both kx and
-kx are stored, each with weight 1 / n; in exact arithmetic T(-kx, 0) = conj(T(kx, 0)) there, and the gradient is DEFINED as the table G with
dL = sum over stored entries (Re G dRe l + Im G dIm l) for every admissible dl that obeys the symmetry itself:
G(kx, 0) = (T(kx, 0) + conj(T(-kx, 0))) / (2 n).  (The first condition alone does not fix G on that line: any split of a pair's cotangent
between its two entries satisfies it.)
"""
import numpy as np

import pspec_linear_adjoint_oracle as A

# deliberately wrong gradients (mutation tests): every lam term dropped (the cotangents of the stage states alone); c D where c conj(D)
# belongs; the stage states of the products shifted by one (s2 where s3 belongs, s1 for s2, s0 for s1); the ky = 0 line left unsymmetrised --
# the cotangent of a pair (kx, -kx) credited to its kx > 0 entry alone, which satisfies the first condition of the definition and not the
# second (with T / n on both entries the line is symmetric up to rounding: that is no mistake a float64 scheme can show); the modes with
# ky > 0 weighted 1 where they stand for 2
WRONG = ('lam_dropped', 'not_conjugated', 'stage_shift', 'line_unsymmetrised', 'mirror_weight_one')


def symmetric_table(rng, S, scale=1.0):
    """A random complex table [nx, nh] (rfft2 layout) with l(-k) = conj(l(k)) on the ky = 0 line and 0 at (0, 0): an admissible perturbation."""
    d = scale * (rng.standard_normal((S.nx, S.ny // 2 + 1)) + 1j * rng.standard_normal((S.nx, S.ny // 2 + 1)))
    line = d[:, 0]
    d[:, 0] = 0.5 * (line + np.conj(line[(-np.arange(S.nx)) % S.nx]))
    d[0, 0] = 0.0
    return d


class OperatorGradScheme(A.LinearAdjointScheme):
    """LinearAdjointScheme whose factors come from ``table`` (complex [nx, nh], rfft2 layout, l = lambda dt / 2) when one is set; None: from
    the parameters, as the parent.  ``parameter_table()`` is the parameters' table and ``parameter_derivatives()`` its partial derivatives."""

    def __init__(self, *args, **kw):
        A.LinearAdjointScheme.__init__(self, *args, **kw)
        self.table = None

    def parameter_table(self):
        return self.linear_operator() * (0.5 * self.dt)

    def parameter_derivatives(self):
        """dict name -> d l / d parameter [nx, nh] for nu, drag, nu_h, mu, beta (the class note's formula, on the kept modes)."""
        h, p, q = 0.5 * self.dt, self.hyper[1], self.hypo[1]
        return dict(nu=-h * self.M * self.k2, drag=-h * self.M, nu_h=-h * self.M * self.k2 ** p, mu=-h * self.M * self.ik2 ** q,
                    beta=1j * h * self.M * self.kx * self.ik2)

    def factors(self):
        if self.table is None:
            return A.LinearAdjointScheme.factors(self)
        return np.exp(self.table), np.exp(2 * self.table)

    def stored_pairing(self, G, dl):
        """sum over the stored entries (every kx, ky >= 0 inside the band) of Re G dRe l + Im G dIm l, per grid."""
        return (G.real * dl.real + G.imag * dl.imag).sum(axis=(-2, -1))

    def finish(self, T, wrong=None):
        """The table gradient G [..., nx, nh] from the raw sum T: the weights and the symmetry of the ky = 0 line (the module note)."""
        n = float(self.nx * self.ny)
        G = T * ((1.0 if wrong == 'mirror_weight_one' else 2.0) / n)
        line = T[..., :, 0]
        if wrong == 'line_unsymmetrised':
            mx = np.fft.fftfreq(self.nx) * self.nx
            G[..., :, 0] = np.where(mx > 0, 2.0, 0.0) * line / n
        else:
            G[..., :, 0] = (line + np.conj(line[..., (-np.arange(self.nx)) % self.nx])) / (2 * n)
        return G

    def operator_vjp(self, w, mean, lam, nsteps=1, t=None, mu=None, starts=None, wrong=()):
        """dict: None -> G [B, nx, nh], the gradient in the table per grid (complex: Re G, Im G the derivatives in Re l, Im l) of
        L = <w(nsteps), lam> (+ <theta(nsteps), mu>), and every name in ``wrong`` -> that deliberately wrong gradient, all from one sweep.
        Arguments as LinearAdjointScheme.step_vjp."""
        bad = set(wrong) - set(WRONG)
        if bad:
            raise ValueError(sorted(bad))
        dt = self.dt
        scalar = t is not None
        E, E2 = self.factors()
        F, F2 = np.conj(E), np.conj(E2)
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
        zero = np.zeros_like(lam)
        raw = ('lam_dropped', 'not_conjugated', 'stage_shift')
        T = {k: np.zeros_like(lam) for k in (None,) + tuple(k for k in raw if k in wrong)}

        def add(r3, r2, r1, lam, s0, s1, s2, s3):
            for k in T:
                a, b, c = (s2, s1, s0) if k == 'stage_shift' else (s3, s2, s1)
                l = zero if k == 'lam_dropped' else lam
                cj = (lambda z: z) if k == 'not_conjugated' else np.conj
                T[k] += (r3 + l / 3) * cj(a + E2 * s0) + r2 * cj(E * s0) + 2.0 / 3.0 * l * cj(E * b) + (r1 + 2.0 / 3.0 * F * l) * cj(c)

        for s in reversed(starts):
            st = self.stages(s[0], mean, s[1]) if scalar else [(x, zero) for x in self.stages(s, mean)]
            s0, s1, s2, s3 = st
            k4, m4 = dt / 6 * lam, dt / 6 * mu
            r3, rt = self.nonlinear_vjp(s3[0], s3[1], mean, k4, m4)
            wbar, tbar = F2 * (lam + r3), Et2 * (mu + rt)
            k3, m3 = dt / 3 * F * lam + dt * F * r3, dt / 3 * Et * mu + dt * Et * rt
            r2, rt = self.nonlinear_vjp(s2[0], s2[1], mean, k3, m3)
            wbar, tbar = wbar + F * r2, tbar + Et * rt
            k2, m2 = dt / 3 * F * lam + dt / 2 * r2, dt / 3 * Et * mu + dt / 2 * rt
            r1, rt = self.nonlinear_vjp(s1[0], s1[1], mean, k2, m2)
            wbar, tbar = wbar + F * r1, tbar + Et * rt
            k1, m1 = dt / 6 * F2 * lam + dt / 2 * F * r1, dt / 6 * Et2 * mu + dt / 2 * Et * rt
            rw, rt = self.nonlinear_vjp(s0[0], s0[1], mean, k1, m1)
            add(r3, r2, r1, lam, s0[0], s1[0], s2[0], s3[0])
            lam, mu = wbar + rw, tbar + rt
        out = {k: self.finish(v) for k, v in T.items()}
        for k in ('line_unsymmetrised', 'mirror_weight_one'):
            if k in wrong:
                out[k] = self.finish(T[None], k)
        return out


def stochastic_operator_vjp(S, amp, seed, w, mean, lam, nsteps, t=None, mu=None, ids=None, n0=0, wrong=()):
    """operator_vjp of the stochastic run: about the noisy trajectory, whose start spectra carry the kicks (the kick does not depend on l)."""
    starts = A.stochastic_starts(S, amp, seed, w, mean, nsteps, t=t, ids=ids, n0=n0)[0]
    return S.operator_vjp(w, mean, lam, nsteps, t=t, mu=mu, starts=starts, wrong=wrong)
