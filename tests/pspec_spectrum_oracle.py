"""NumPy float64 restatement (tests only) of the shell spectra and spectral transfers of the pseudo-spectral periodic solver
(csrc/pspec_kernels.hip: nns_spec_ns_shells, nns_spec_ns_spectrum_f32, nns_spec_ns_transfer_f32; nns.periodic.PeriodicSolver.spectrum /
transfer / energy_budget), on the schemes of tests/pspec_oracle.py, tests/pspec_forced_oracle.py and tests/pspec_scalar_oracle.py.

Spectra are unnormalised rfft2 spectra [..., nx, nh]; the stored modes are the kept ones (3|m_x| < nx, j < my1), n = nx ny,
wt = 1 on the j = 0 line and 2 on j > 0.
  Shells: dk = min(2 pi / Lx, 2 pi / Ly); the mode k belongs to shell s = floor(|k| / dk + 1/2); S = floor(k_max / dk + 1/2) + 1 with k_max the
  band's corner, hypot(2 pi / Lx ((nx - 1) // 3), 2 pi / Ly (my1 - 1)); centres k_s = s dk; the (0, 0) mode contributes nothing.
  Per shell, sum over its stored modes of wt (...) / n^2:
      E = 1/2 |w^|^2 / |k|^2,  Z = 1/2 |w^|^2,  F = Re(conj psi^ g^) (psi^ = w^ / |k|^2; 0 without a force),  V = 1/2 |theta^|^2 (k != 0)
      T_Z = Re(conj w^ N^),  T_E = Re(conj w^ N^) / |k|^2,  N^ = -M rfft2(u w_x + v w_y) in the co-moving frame (U0 = V0 = 0)
      T_theta = Re(conj theta^ N_theta^) (k != 0),  N_theta^ = -M_theta rfft2(u theta_x + v theta_y): advection alone, G taken as 0
  Budget: dE(s)/dt = T_E(s) + F(s) - 2 nu Z(s) - 2 alpha E(s).
  Absolute scales (what a relative error of the nonlinear term moves a shell by): A_E = sum wt |psi^| |N^| / n^2, A_Z with |w^|, A_theta with
  |theta^| |N_theta^|, A_F = sum wt |psi^| |g^| / n^2.
"""
import numpy as np

import pspec_oracle as O

# deliberately wrong definitions (mutation tests): 'floor': s = floor(|k| / dk); 'weight1': wt = 1 on j > 0 too; 'dkmax': dk = max of the two;
# 'noik2': the 1 / |k|^2 of E, F and T_E missing; 'sign': N^ with the wrong sign; 'grad': the scalar's mean gradient left in N_theta^
MUTATIONS = ('floor', 'weight1', 'dkmax', 'noik2', 'sign', 'grad')


def shells(nx, ny, Lx, Ly, mutate=None):
    """(k [S], dk, S): shell centres, width and count of the box."""
    kx1, ky1 = 2 * np.pi / Lx, 2 * np.pi / Ly
    dk = max(kx1, ky1) if mutate == 'dkmax' else min(kx1, ky1)
    kmax = np.hypot(kx1 * ((nx - 1) // 3), ky1 * (O.kept_y(ny) - 1))
    S = int(np.floor(kmax / dk + 0.5)) + 1
    return dk * np.arange(S, dtype=np.float64), dk, S


def shell_position(Sc, mutate=None):
    """|k| / dk + 1/2 [nx, nh] of every mode: its integer part is the shell."""
    dk = shells(Sc.nx, Sc.ny, Sc.Lx, Sc.Ly, mutate)[1]
    return np.sqrt(Sc.k2) / dk + (0.0 if mutate == 'floor' else 0.5)


def boundary_distance(Sc):
    """The least distance, in shell widths, of a kept mode from a shell boundary."""
    p = shell_position(Sc)[Sc.M > 0]
    f = p - np.floor(p)
    return float(np.minimum(f, 1.0 - f).min())


def bin_shells(Sc, f, mutate=None):
    """[..., S] per-shell sums of wt f / n^2 over the kept modes of the real per-mode array f [..., nx, nh]; S is the unmutated count."""
    S = shells(Sc.nx, Sc.ny, Sc.Lx, Sc.Ly)[2]
    keep = Sc.M > 0
    idx = np.floor(shell_position(Sc, mutate)).astype(np.int64)[keep]
    assert idx.max() < S
    wt = np.where(np.arange(Sc.ny // 2 + 1) == 0, 1.0, 1.0 if mutate == 'weight1' else 2.0)[None, :]
    v = (wt * f / float(Sc.nx * Sc.ny) ** 2)[..., keep]
    lead = v.shape[:-1]
    v = v.reshape(-1, v.shape[-1])
    out = np.stack([np.bincount(idx, weights=row, minlength=S) for row in v])
    return out.reshape(lead + (S,))


def _ik2(Sc, mutate):
    return (Sc.k2 > 0).astype(np.float64) if mutate == 'noik2' else Sc.ik2


def spectrum(Sc, w, t=None, mutate=None):
    """dict E, Z, F, V (V None without t), each [..., S], and the scale A_F; the force is Sc.g (F = 0 without one)."""
    a2 = w.real ** 2 + w.imag ** 2
    ik2 = _ik2(Sc, mutate)
    g = getattr(Sc, 'g', None)
    r = dict(E=bin_shells(Sc, 0.5 * a2 * ik2, mutate), Z=bin_shells(Sc, 0.5 * a2, mutate), V=None)
    if g is None:
        r['F'] = np.zeros_like(r['E'])
        r['A_F'] = np.zeros_like(r['E'])
    else:
        r['F'] = bin_shells(Sc, ik2 * (np.conj(w) * g).real, mutate)
        r['A_F'] = bin_shells(Sc, Sc.ik2 * np.abs(w) * np.abs(g))
    if t is not None:
        r['V'] = bin_shells(Sc, 0.5 * (t.real ** 2 + t.imag ** 2), mutate)           # the (0, 0) mode is outside M
    return r


def nonlinear_terms(Sc, w, t=None, mutate=None):
    """(N^, N_theta^ or None) in the co-moving frame; the scalar's without its mean gradient ('grad': with Sc.grad)."""
    zero = np.zeros(w.shape[:-2] + (2,))
    sgn = -1.0 if mutate == 'sign' else 1.0
    N = sgn * O.Scheme.nonlinear(Sc, w, zero)
    if t is None:
        return N, None
    uh, vh = Sc.velocity_hat(w, zero)
    u, v = Sc.irfft2(uh), Sc.irfft2(vh)
    gx, gy = Sc.grad if mutate == 'grad' else (0.0, 0.0)
    tx, ty = Sc.irfft2(1j * Sc.kx * t), Sc.irfft2(1j * Sc.ky * t)
    return N, -sgn * Sc.MNt * np.fft.rfft2(u * (tx + gx) + v * (ty + gy))


def transfer(Sc, w, t=None, mutate=None):
    """dict T_E, T_Z, T_theta (None without t), each [..., S], and the scales A_E, A_Z, A_theta (unmutated definitions)."""
    N, Nt = nonlinear_terms(Sc, w, t, mutate)
    wn = (np.conj(w) * N).real
    r = dict(T_E=bin_shells(Sc, wn * _ik2(Sc, mutate), mutate), T_Z=bin_shells(Sc, wn, mutate), T_theta=None, A_theta=None,
             A_E=bin_shells(Sc, Sc.ik2 * np.abs(w) * np.abs(N)), A_Z=bin_shells(Sc, np.abs(w) * np.abs(N)))
    if t is not None:
        r['T_theta'] = bin_shells(Sc, (np.conj(t) * Nt).real, mutate)
        r['A_theta'] = bin_shells(Sc, np.abs(t) * np.abs(Nt))
    return r


def energy_budget(Sc, w, mutate=None):
    """dE(s)/dt = T_E + F - 2 nu Z - 2 alpha E, [..., S], and its scale A_E + A_F + 2 nu Z + 2 alpha E."""
    sp, tr = spectrum(Sc, w, None, mutate), transfer(Sc, w, None, mutate)
    drag = getattr(Sc, 'drag', 0.0)
    rhs = tr['T_E'] + sp['F'] - 2 * Sc.nu * sp['Z'] - 2 * drag * sp['E']
    return rhs, tr['A_E'] + sp['A_F'] + 2 * Sc.nu * sp['Z'] + 2 * drag * sp['E']
