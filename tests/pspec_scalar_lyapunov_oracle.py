"""NumPy float64 restatement (tests only) of K tangent pairs on one base with a scalar and of the Lyapunov spectrum built on them
(csrc/pspec_scalar_tangents.hip: nns_spec_ns_step_scalar_tangents_f32, nns_spec_ns_tangent_variance_gram_f64; nns.periodic.PeriodicSolver.
step_tangents_scalar / tangent_gram_scalar / orthonormalize_tangents_scalar / lyapunov_spectrum_scalar): K calls of
pspec_scalar_tangent_oracle.ScalarTangentScheme.step_jvp, the Gram matrix of the weighted inner product of pairs (a_w, a_t), (b_w, b_t)

    <a, b> = 1/2 sum_modes wt Re(conj(a_w) b_w) / |k|^2 / (nx ny)^2 + scalar_weight 1/2 sum_modes' wt Re(conj(a_t) b_t) / (nx ny)^2

(the kept modes of the rfft2 half spectrum, wt 1 on j = 0 and 2 on j > 0; the second sum without the (0, 0) mode: the mean of dtheta does not
enter), whose diagonal is E(dw) + scalar_weight 1/2 <dtheta'^2>, the norm of lyapunov_exponent_scalar; the factorisation D = Q R under it
(modified Gram-Schmidt, done twice: not the solver's Cholesky QR, so the two check each other; both halves of a pair are combined with the
same coefficients, the (0, 0) entries of dtheta^ included) and the finite-time exponents as in pspec_lyapunov_oracle.
"""
import numpy as np

# deliberately wrong spectra (mutation tests): each pair scaled to unit norm without projection; the inner product without the scalar's half
# (the energy alone); the (0, 0) mode of dtheta^ counted in it; a Cholesky QR done twice whose second pass's logs are dropped; member k's
# stages fed with member 0's dN_theta; scalar_weight taken as 1
WRONG = ('normalise_only', 'no_scalar_in_product', 'mean_in_product', 'first_pass_logs', 'shared_accumulator', 'weight_ignored')


class ScalarLyapunov(object):
    """scheme: a pspec_scalar_tangent_oracle.ScalarTangentScheme (the right one).  weight: scalar_weight > 0.  wrong: None, or one of WRONG.
    Tangent pairs are two complex128 arrays [K, ..., nx, nh]."""

    def __init__(self, scheme, weight=1.0, wrong=None):
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.S, self.weight, self.wrong = scheme, float(weight), wrong

    def weights(self):
        """(the real weight of a stored mode of dw^, that of dtheta^) in <a, b>: [nx, nh] each."""
        S = self.S
        nh = S.ny // 2 + 1
        wt = np.full((S.nx, nh), 2.0)
        wt[:, 0] = 1.0
        k2 = S.kx ** 2 + S.ky ** 2 + np.zeros((S.nx, nh))
        inv = np.where(k2 > 0, 1.0 / np.where(k2 > 0, k2, 1.0), 0.0)
        n2 = (float(S.nx) * S.ny) ** 2
        ww = 0.5 * wt * inv * (S.M > 0) * (k2 > 0) / n2
        sw = 1.0 if self.wrong == 'weight_ignored' else 0.0 if self.wrong == 'no_scalar_in_product' else self.weight
        keep = (S.Mt > 0) if self.wrong == 'mean_in_product' else (S.Mt > 0) * (k2 > 0)
        return ww, sw * 0.5 * wt * keep / n2

    def gram(self, Dw, Dt):
        """[..., K, K] of the pairs (Dw, Dt) [K, ..., nx, nh]."""
        ww, wq = self.weights()
        return (np.einsum('k...ij,l...ij,ij->...kl', Dw.conj(), Dw, ww) + np.einsum('k...ij,l...ij,ij->...kl', Dt.conj(), Dt, wq)).real

    def dot(self, aw, at, bw, bt):
        """<a, b> per grid, shaped to multiply a spectrum: [..., 1, 1]."""
        ww, wq = self.weights()
        return (np.einsum('...ij,...ij,ij->...', aw.conj(), bw, ww) + np.einsum('...ij,...ij,ij->...', at.conj(), bt, wq)).real[..., None, None]

    def qr(self, Dw, Dt):
        """(Qw, Qt, log diag R [..., K]) of D = Q R under the inner product, R upper triangular with a positive diagonal."""
        Dw, Dt = np.array(Dw, dtype=np.complex128), np.array(Dt, dtype=np.complex128)
        K = Dw.shape[0]
        if self.wrong == 'first_pass_logs':
            logs = None
            for _ in range(2):
                L = np.linalg.cholesky(self.gram(Dw, Dt))                              # gram = L L^T, R = L^T
                Rinv = np.linalg.inv(np.swapaxes(L, -1, -2))
                Dw = np.einsum('l...ij,...lk->k...ij', Dw, Rinv)
                Dt = np.einsum('l...ij,...lk->k...ij', Dt, Rinv)
                if logs is None:
                    logs = np.log(np.diagonal(L, axis1=-2, axis2=-1))
            return Dw, Dt, logs
        Qw, Qt = Dw.copy(), Dt.copy()
        diag = []
        for k in range(K):
            if self.wrong != 'normalise_only':
                for _ in range(2):
                    for l in range(k):
                        p = self.dot(Qw[l], Qt[l], Qw[k], Qt[k])
                        Qw[k], Qt[k] = Qw[k] - p * Qw[l], Qt[k] - p * Qt[l]
            r = np.sqrt(self.dot(Qw[k], Qt[k], Qw[k], Qt[k]))
            Qw[k], Qt[k] = Qw[k] / r, Qt[k] / r
            diag.append(r[..., 0, 0])
        return Qw, Qt, np.log(np.stack(diag, axis=-1))

    def advance(self, w, t, mean, Dw, Dt, nsteps, starts=None):
        """(Dw, Dt) after nsteps steps from (w, t): step_jvp of every member (starts: the start spectra (w, t) of those steps of a stochastic run)."""
        S = self.S
        if self.wrong != 'shared_accumulator':
            out = [S.step_jvp(w, t, mean, dw, dq, nsteps, starts=starts) for dw, dq in zip(Dw, Dt)]
            return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        h = S.dt
        E, E2 = S.factors()
        Et, Et2 = S.scalar_factors()
        mw, mt = S.tangent_masks()
        if starts is None:
            starts = []
            for _ in range(nsteps):
                starts.append((w, t))
                w, t = S.step(w, t, mean, 1)
        Dw, Dt = mw * np.array(Dw, dtype=np.complex128), mt * np.array(Dt, dtype=np.complex128)
        K = len(Dw)

        def jvp(s, dws, dqs):                                                          # every dN_theta is member 0's
            r = [S.nonlinear_jvp(s[0], s[1], mean, dws[k], dqs[k]) for k in range(K)]
            return np.stack([x[0] for x in r]), np.stack([r[0][1]] * K)
        for w0, t0 in starts:
            s = S.stages(w0, mean, t0)
            a, at = jvp(s[0], Dw, Dt)
            b, bt = jvp(s[1], E * (Dw + h / 2 * a), Et * (Dt + h / 2 * at))
            c, ct = jvp(s[2], E * Dw + h / 2 * b, Et * Dt + h / 2 * bt)
            d, dth = jvp(s[3], E2 * Dw + h * E * c, Et2 * Dt + h * Et * ct)
            Dw = E2 * Dw + h / 6 * (E2 * a + 2 * E * (b + c) + d)
            Dt = Et2 * Dt + h / 6 * (Et2 * at + 2 * Et * (bt + ct) + dth)
        return Dw, Dt

    def exponents(self, w, t, mean, Dw, Dt, nsteps, every, starts=None):
        """(lambda [..., K], Qw, Qt): the finite-time exponents over nsteps steps from (w, t) with the pairs (Dw, Dt), orthonormalised at
        the start and after every `every` steps, and the orthonormal pairs at the end.  starts: the nsteps start spectra of a stochastic run."""
        S = self.S
        Dw, Dt = self.qr(Dw, Dt)[:2]
        total, done = 0.0, 0
        while done < nsteps:
            n = min(every, nsteps - done)
            Dw, Dt = self.advance(w, t, mean, Dw, Dt, n, None if starts is None else starts[done:done + n])
            if starts is None:
                w, t = S.step(w, t, mean, n)
            Dw, Dt, logs = self.qr(Dw, Dt)
            total = total + logs
            done += n
        return total / (nsteps * S.dt), Dw, Dt
