"""NumPy float64 restatement (tests only) of K tangents on one base and of the Lyapunov spectrum built on them (csrc/pspec_kernels.hip:
nns_spec_ns_step_tangents_f32, nns_spec_ns_tangent_gram_f64, nns_spec_ns_tangent_combine_f32; nns.periodic.PeriodicSolver.step_tangents /
tangent_gram / orthonormalize_tangents / lyapunov_spectrum): K calls of pspec_tangent_oracle.TangentScheme.step_jvp, the Gram matrix of the
energy inner product

    <a, b> = 1/2 sum_modes wt Re(conj(a) b) / |k|^2 / (nx ny)^2        (the kept modes of the rfft2 half spectrum; wt 1 on j = 0, 2 on j > 0)

whose diagonal is the energy 1/2 <|du|^2> of a perturbation, the factorisation D = Q R under it (modified Gram-Schmidt, done twice: not
the solver's Cholesky QR, so the two check each other) and the finite-time exponents: the vectors are orthonormalised at the start and
after every segment of `every` steps, and lambda_k = sum over the segments of log R_kk / (nsteps dt).
"""
import numpy as np

# deliberately wrong spectra (mutation tests): each vector scaled to unit energy without projection; the inner product without 1 / |k|^2 (the
# enstrophy's); a Cholesky QR done twice whose second pass's logs are dropped; the first segment's growth measured from the raw vectors;
# tangent k's stages fed with tangent 0's dN
WRONG = ('normalise_only', 'enstrophy_product', 'first_pass_logs', 'no_initial_orthonormalisation', 'shared_accumulator')


class Lyapunov(object):
    """scheme: a pspec_tangent_oracle.TangentScheme (the right one).  wrong: None, or one of WRONG.  Tangents are complex128 [K, ..., nx, nh]."""

    def __init__(self, scheme, wrong=None):
        if wrong is not None and wrong not in WRONG:
            raise ValueError(wrong)
        self.S, self.wrong = scheme, wrong

    def weight(self):
        """The real weight of a stored mode in <a, b> = sum weight Re(conj(a) b): [nx, nh]."""
        S = self.S
        nh = S.ny // 2 + 1
        wt = np.full((S.nx, nh), 2.0)
        wt[:, 0] = 1.0
        k2 = S.kx ** 2 + S.ky ** 2 + np.zeros((S.nx, nh))
        inv = np.ones_like(k2) if self.wrong == 'enstrophy_product' else np.where(k2 > 0, 1.0 / np.where(k2 > 0, k2, 1.0), 0.0)
        return 0.5 * wt * inv * (S.M > 0) * (k2 > 0) / (float(S.nx) * S.ny) ** 2

    def gram(self, D):
        """[..., K, K] of D [K, ..., nx, nh]."""
        W = self.weight()
        return np.einsum('k...ij,l...ij,ij->...kl', D.conj(), D, W).real

    def qr(self, D):
        """(Q, log diag R [..., K]) of D = Q R under the inner product, R upper triangular with a positive diagonal."""
        D = np.array(D, dtype=np.complex128)
        W = self.weight()
        dot = lambda a, b: np.einsum('...ij,...ij,ij->...', a.conj(), b, W).real[..., None, None]
        K = D.shape[0]
        if self.wrong == 'first_pass_logs':
            logs = None
            for _ in range(2):
                L = np.linalg.cholesky(self.gram(D))                                   # gram = L L^T, R = L^T
                Rinv = np.linalg.inv(np.swapaxes(L, -1, -2))
                D = np.einsum('l...ij,...lk->k...ij', D, Rinv)
                if logs is None:
                    logs = np.log(np.diagonal(L, axis1=-2, axis2=-1))
            return D, logs
        Q = D.copy()
        diag = []
        for k in range(K):
            if self.wrong != 'normalise_only':
                for _ in range(2):
                    for l in range(k):
                        Q[k] = Q[k] - dot(Q[l], Q[k]) * Q[l]
            r = np.sqrt(dot(Q[k], Q[k]))
            Q[k] = Q[k] / r
            diag.append(r[..., 0, 0])
        return Q, np.log(np.stack(diag, axis=-1))

    def advance(self, w, mean, D, nsteps, starts=None):
        """D after nsteps steps from w: step_jvp of every member (starts: the start spectra of those steps of a stochastic run)."""
        S = self.S
        if self.wrong != 'shared_accumulator':
            return np.stack([S.step_jvp(w, mean, d, nsteps, starts=starts) for d in D])
        dt = S.dt
        E, E2 = S.factors()
        if starts is None:
            starts = []
            for _ in range(nsteps):
                starts.append(w)
                w = S.step(w, mean, 1)
        D = S.M * np.array(D, dtype=np.complex128)
        for w0 in starts:
            s = S.stages(w0, mean)
            da = S.nonlinear_jvp(s[0], mean, D[0])                                      # every dN is member 0's
            db = S.nonlinear_jvp(s[1], mean, E * (D[0] + dt / 2 * da))
            dc = S.nonlinear_jvp(s[2], mean, E * D[0] + dt / 2 * db)
            dd = S.nonlinear_jvp(s[3], mean, E2 * D[0] + dt * E * dc)
            D = E2 * D + dt / 6 * (E2 * da + 2 * E * (db + dc) + dd)
        return D

    def exponents(self, w, mean, D, nsteps, every, starts=None):
        """(lambda [..., K], Q): the finite-time exponents over nsteps steps from w with the tangents D, orthonormalised at the start and
        after every `every` steps, and the orthonormal vectors at the end.  starts: the nsteps start spectra of a stochastic run."""
        S = self.S
        D = np.array(D, dtype=np.complex128)
        if self.wrong != 'no_initial_orthonormalisation':
            D = self.qr(D)[0]
        total, done = 0.0, 0
        while done < nsteps:
            n = min(every, nsteps - done)
            D = self.advance(w, mean, D, n, None if starts is None else starts[done:done + n])
            if starts is None:
                w = S.step(w, mean, n)
            D, logs = self.qr(D)
            total = total + logs
            done += n
        return total / (nsteps * S.dt), D


def kaplan_yorke(lam):
    """The Kaplan-Yorke dimension of one spectrum (1-D): j + S_j / |lambda_(j+1)|, j the largest count with S_j >= 0; len(lam) when all are."""
    lam = np.sort(np.asarray(lam, dtype=np.float64))[::-1]
    S = np.concatenate([[0.0], np.cumsum(lam)])
    j = max(i for i in range(len(lam) + 1) if S[i] >= 0)
    return float(j) if j == len(lam) else j + S[j] / abs(lam[j])
