"""NumPy restatement (tests only) of the white-in-time stochastic forcing of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_stochastic_f32; nns.periodic.PeriodicSolver.set_stochastic_forcing / ring_forcing / stochastic_injection), on the schemes of
tests/pspec_forced_oracle.py, tests/pspec_scalar_oracle.py and tests/pspec_buoyant_oracle.py.

After the complete deterministic Lawson-RK4 step n of the scheme (drag, steady force, scalar, buoyancy: whichever it has) the vorticity spectrum
gets one kick (additive noise: no Ito / Stratonovich ambiguity), the scalar none:

    w^_k  <-  w^_k + sqrt(dt) a_k xi_k(n, id_b)                    on the kept modes k != (0, 0)

a: a non-negative float32 table over the stored modes [my1][nx] (one grid of the solver's state layout), shared by the batch.
xi: complex standard normal, E |xi|^2 = 1, independent over stored modes, steps n and grid ids, from Philox4x32-10 (Salmon, Moraes, Dror, Shaw,
SC'11) in integers: key = (seed low word, seed high word), counter = (n low, n high, mode, id_b), mode = j nx + i (i the fftfreq-order x index);
of the outputs x0, x1 are used:  u1 = ((x0 >> 8) + 1) 2^-24 in (0, 1],  u2 = (x1 >> 8) 2^-24 in [0, 1),  xi = sqrt(-ln u1) exp(2 pi i u2).
The stored j = 0 line holds +m_x and -m_x, which must stay conjugate: the element of -m_x takes the counter of |m_x| and is conjugated.

Table of a mean injection rate eps_s per shell (the shells of tests/pspec_spectrum_oracle.py): a_k = |k| nx ny sqrt(2 eps_s / N_s), N_s the
number of full-spectrum modes of the shell inside the kept band (wt = 1 per stored mode on j = 0, 2 on j > 0); then the mean energy input is
    eps = 1/2 sum_stored wt a_k^2 / (|k|^2 (nx ny)^2) = sum_s eps_s
exactly and independently of the state (E |xi|^2 = 1; energy = 1/2 sum wt |w^|^2 / (|k|^2 (nx ny)^2)).
"""
import numpy as np

import pspec_oracle as O
import pspec_spectrum_oracle as SP

# deliberately wrong schemes (mutation tests): 'nosqrtdt': the kick without sqrt(dt); 'var1': variance 1 per component (E |xi|^2 = 2);
# 'noconj': the j = 0 mirror takes |m_x|'s sample unconjugated; 'before': the kick before the deterministic step instead of after it
MUTATIONS = ('nosqrtdt', 'var1', 'noconj', 'before')

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 on integer arrays: counter [..., 4], key [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., q] for q in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def uniforms(x):
    """(u1 in (0, 1], u2 in [0, 1)) float64 from Philox outputs x [..., 4] (x0 and x1; x2, x3 are discarded)."""
    x = np.asarray(x, dtype=np.uint64)
    return ((x[..., 0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24, (x[..., 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normals(x):
    """Complex standard normal, E |xi|^2 = 1, float64, from Philox outputs x [..., 4]."""
    u1, u2 = uniforms(x)
    return np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)


def xi_stored(nx, ny, seed, n, ids, mutate=None, where=None):
    """xi [B, my1, nx] (complex128) of step n for the grid ids `ids` [B], in the solver's state layout: every stored element, or only those of
    the mask `where` [my1, nx] (zero elsewhere; the kernel draws only where the mode is kept and a != 0)."""
    my1 = O.kept_y(ny)
    mx = (np.fft.fftfreq(nx) * nx).astype(np.int64)
    i, j = np.arange(nx, dtype=np.int64)[None, :], np.arange(my1, dtype=np.int64)[:, None]
    mirror = (j == 0) & (mx[None, :] < 0)
    mode = j * nx + np.where(mirror, -mx[None, :], i)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 1)
    where = np.ones(mode.shape, dtype=bool) if where is None else np.asarray(where, dtype=bool)
    counter = np.stack(np.broadcast_arrays(np.int64(n & 0xFFFFFFFF), np.int64((n >> 32) & 0xFFFFFFFF), mode[where][None], ids), axis=-1)
    xi = normals(philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])))
    if mutate == 'var1':
        xi = xi * np.sqrt(2.0)
    if mutate != 'noconj':
        xi = np.where(mirror[where][None], np.conj(xi), xi)
    out = np.zeros((ids.shape[0],) + mode.shape, dtype=np.complex128)
    out[:, where] = xi
    return out


def stored_grid(nx, ny, Lx, Ly):
    """(|k|^2 [my1, nx], kept [my1, nx] bool, wt [my1, 1], shell [my1, nx]) of the stored modes: the 2/3 mask without (0, 0), the weights and the
    shell predicate floor(|k| / dk + 1/2) in float64."""
    my1 = O.kept_y(ny)
    mx = np.fft.fftfreq(nx) * nx
    j = np.arange(my1, dtype=np.float64)
    kx, ky = (2 * np.pi / Lx * mx)[None, :], (2 * np.pi / Ly * j)[:, None]
    k2 = kx * kx + ky * ky
    dk = SP.shells(nx, ny, Lx, Ly)[1]
    return k2, (3 * np.abs(mx)[None, :] < nx) & (k2 > 0), np.where(j == 0, 1.0, 2.0)[:, None], np.floor(np.sqrt(k2) / dk + 0.5).astype(np.int64)


def mode_counts(nx, ny, Lx, Ly):
    """N_s [S]: the full-spectrum modes of every shell inside the kept band."""
    S = SP.shells(nx, ny, Lx, Ly)[2]
    k2, kept, wt, shell = stored_grid(nx, ny, Lx, Ly)
    return np.bincount(shell[kept], weights=np.broadcast_to(wt, shell.shape)[kept], minlength=S)


def amplitude_table(nx, ny, Lx, Ly, rate_by_shell):
    """a float32 [my1, nx] for the mean injection rates eps_s [S]: a_k = |k| nx ny sqrt(2 eps_s / N_s) on the kept modes, 0 elsewhere."""
    rate = np.asarray(rate_by_shell, dtype=np.float64)
    k2, kept, wt, shell = stored_grid(nx, ny, Lx, Ly)
    count = mode_counts(nx, ny, Lx, Ly)
    assert rate.shape == count.shape and not np.any((rate > 0) & (count == 0))
    per_mode = np.where(count > 0, 2.0 * rate / np.maximum(count, 1.0), 0.0)
    return np.where(kept, np.sqrt(k2) * (nx * ny) * np.sqrt(per_mode[np.minimum(shell, len(count) - 1)]), 0.0).astype(np.float32)


def ring_rates(nx, ny, Lx, Ly, rate, k_lo, k_hi):
    """eps_s [S]: `rate` shared by the shells with k_lo <= k_s <= k_hi in proportion to their mode counts."""
    k = SP.shells(nx, ny, Lx, Ly)[0]
    count = np.where((k >= k_lo) & (k <= k_hi), mode_counts(nx, ny, Lx, Ly), 0.0)
    return rate * count / count.sum()


def injection(nx, ny, Lx, Ly, amp):
    """The exact mean injection per shell [S] of a table amp [my1, nx]: 1/2 sum wt a^2 / (|k|^2 (nx ny)^2)."""
    S = SP.shells(nx, ny, Lx, Ly)[2]
    k2, kept, wt, shell = stored_grid(nx, ny, Lx, Ly)
    a = np.asarray(amp, dtype=np.float64)
    e = 0.5 * wt * a * a / (np.where(kept, k2, 1.0) * float(nx * ny) ** 2)
    return np.bincount(shell[kept], weights=e[kept], minlength=S)


def kick_stored(nx, ny, dt, amp, seed, n, ids, mutate=None):
    """sqrt(dt) a xi [B, my1, nx] (complex128) of step n on the kept modes, zero elsewhere."""
    a = np.where(stored_grid(nx, ny, 1.0, 1.0)[1], np.asarray(amp, dtype=np.float64), 0.0)
    s = 1.0 if mutate == 'nosqrtdt' else np.sqrt(dt)
    return s * a[None] * xi_stored(nx, ny, seed, n, ids, mutate, where=a != 0)


class Stochastic(object):
    """Steps any scheme S of the sibling oracles (ForcedScheme and its scalar and buoyant descendants) one step at a time and adds the kick.
    amp: the float32 table [my1, nx]; ids: the grid ids [B] (default arange(B)); n0: the index of the first step."""

    def __init__(self, S, amp, seed=0, mutate=None):
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError("mutate must be None or one of %s" % (MUTATIONS,))
        self.S, self.amp, self.seed, self.mutate = S, np.asarray(amp, dtype=np.float32), int(seed), mutate

    def kick(self, n, ids):
        """The kick of step n in the schemes' rfft2 layout [B, nx, nh]."""
        return self.S.expand(kick_stored(self.S.nx, self.S.ny, self.S.dt, self.amp, self.seed, n, ids, self.mutate))

    def step(self, w, mean, nsteps=1, t=None, ids=None, n0=0):
        """w (and t, with a scalar) after nsteps steps: w [B, nx, nh]."""
        ids = np.arange(w.shape[0]) if ids is None else ids
        for n in range(n0, n0 + nsteps):
            if self.mutate == 'before':
                w = w + self.kick(n, ids)
            if t is None:
                w = self.S.step(w, mean, 1)
            else:
                w, t = self.S.step(w, t, mean, 1)
            if self.mutate != 'before':
                w = w + self.kick(n, ids)
        return w if t is None else (w, t)
