"""NumPy float64 restatement (tests only) of the pseudo-spectral periodic Navier-Stokes solver of csrc/pspec_kernels.hip
(nns.periodic.PeriodicSolver).

Box [0, Lx) x [0, Ly), fields [..., nx, ny] (axis -2 = x).  Spectra in numpy.fft.rfft2 layout [..., nx, ny // 2 + 1], unnormalised.
  kx = 2 pi m_x / Lx, ky = 2 pi m_y / Ly (m = the fftfreq index);  M = 1 where 3|m_x| < nx and 3|m_y| < ny (drops the Nyquist modes).
  State: w^ (vorticity, M w^ = w^, w^(0,0) = 0) and the mean velocity (U0, V0) [..., 2].
  psi^ = w^ / |k|^2 (0 at k = 0);  u = U0 + irfft2(i ky psi^),  v = V0 - irfft2(i kx psi^)   (w = v_x - u_y).
  N(w^) = -M rfft2(u w_x + v w_y), w_x, w_y spectral.
  Lawson RK4, L = -nu |k|^2, E = exp(L dt / 2):
      a = N(w);  b = N(E (w + dt/2 a));  c = N(E w + dt/2 b);  d = N(E^2 w + dt E c)
      w <- E^2 w + dt/6 (E^2 a + 2 E (b + c) + d)
  init(u, v): w^ = M (i kx v^ - i ky u^), (U0, V0) = grid means: the divergence-free, band-limited projection of (u, v).
  fields: p^ = -M rfft2(2 rho (u_x v_y - u_y v_x)) / |k|^2, p^(0,0) = 0, derivatives from psi^.
"""
import numpy as np


def kept_y(ny):
    return (ny - 1) // 3 + 1


def band(nx, ny, widen=(0, 0)):
    """The 2/3-rule mask [nx, nh] (bool, (0, 0) dropped); widen = (wx, wy) keeps wx more |m_x| and wy more m_y (mutation tests)."""
    mx = np.fft.fftfreq(nx) * nx
    my = np.arange(ny // 2 + 1)
    M = (3 * (np.abs(mx)[:, None] - widen[0]) < nx) & (my[None, :] < kept_y(ny) + widen[1])
    M[0, 0] = False
    return M


def grid(nx, ny, Lx, Ly):
    """kx [nx, 1], ky [1, nh], |k|^2, mask M (float), 1 / |k|^2 (0 at k = 0)."""
    mx = np.fft.fftfreq(nx) * nx
    my = np.arange(ny // 2 + 1)
    kx = (2 * np.pi / Lx * mx)[:, None]
    ky = (2 * np.pi / Ly * my)[None, :]
    k2 = kx * kx + ky * ky
    M = band(nx, ny).astype(np.float64)
    ik2 = np.where(k2 > 0, 1.0 / np.where(k2 > 0, k2, 1.0), 0.0)
    return kx, ky, k2, M, ik2


class Scheme(object):
    """widen: a deliberately wrong dealiasing mask for the nonlinear term of the step (see band); init and fields keep the 2/3 rule."""

    def __init__(self, nx, ny, dt, rho, nu, Lx=2 * np.pi, Ly=2 * np.pi, widen=(0, 0)):
        self.nx, self.ny, self.dt, self.rho, self.nu, self.Lx, self.Ly = nx, ny, dt, rho, nu, Lx, Ly
        self.kx, self.ky, self.k2, self.M, self.ik2 = grid(nx, ny, Lx, Ly)
        self.MN = self.M if tuple(widen) == (0, 0) else band(nx, ny, widen).astype(np.float64)

    def irfft2(self, f):
        return np.fft.irfft2(f, s=(self.nx, self.ny))

    def init(self, u, v):
        u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
        uh, vh = np.fft.rfft2(u), np.fft.rfft2(v)
        w = self.M * (1j * self.kx * vh - 1j * self.ky * uh)
        mean = np.stack([u.mean(axis=(-2, -1)), v.mean(axis=(-2, -1))], axis=-1)
        return w, mean

    def velocity_hat(self, w, mean):
        psi = w * self.ik2
        uh, vh = 1j * self.ky * psi, -1j * self.kx * psi
        n = self.nx * self.ny
        uh[..., 0, 0] = mean[..., 0] * n
        vh[..., 0, 0] = mean[..., 1] * n
        return uh, vh

    def nonlinear(self, w, mean):
        uh, vh = self.velocity_hat(w, mean)
        u, v = self.irfft2(uh), self.irfft2(vh)
        wx, wy = self.irfft2(1j * self.kx * w), self.irfft2(1j * self.ky * w)
        return -self.MN * np.fft.rfft2(u * wx + v * wy)

    def step(self, w, mean, nsteps=1):
        dt = self.dt
        E = np.exp(-self.nu * self.k2 * dt / 2)
        E2 = np.exp(-self.nu * self.k2 * dt)
        for _ in range(nsteps):
            a = self.nonlinear(w, mean)
            b = self.nonlinear(E * (w + dt / 2 * a), mean)
            c = self.nonlinear(E * w + dt / 2 * b, mean)
            d = self.nonlinear(E2 * w + dt * E * c, mean)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
        return w

    def fields(self, w, mean):
        uh, vh = self.velocity_hat(w, mean)
        u, v = self.irfft2(uh), self.irfft2(vh)
        ux, uy = self.irfft2(1j * self.kx * uh), self.irfft2(1j * self.ky * uh)
        vx, vy = self.irfft2(1j * self.kx * vh), self.irfft2(1j * self.ky * vh)
        q = 2 * self.rho * (ux * vy - uy * vx)
        p = self.irfft2(-self.M * np.fft.rfft2(q) * self.ik2)
        return u, v, p

    def simulate(self, u0, v0, nsteps, save_every=1):
        w, mean = self.init(u0, v0)
        out = [self.fields(w, mean)]
        for _ in range(nsteps // save_every):
            w = self.step(w, mean, save_every)
            out.append(self.fields(w, mean))
        return tuple(np.stack([f[i] for f in out]) for i in range(3))

    # ---- diagnostics
    def divergence(self, u, v):
        uh, vh = np.fft.rfft2(u), np.fft.rfft2(v)
        return self.irfft2(1j * self.kx * uh + 1j * self.ky * vh)

    def energy(self, w, mean):
        u, v, _ = self.fields(w, mean)
        return 0.5 * (u * u + v * v).mean(axis=(-2, -1))

    def enstrophy(self, w):
        return 0.5 * (self.irfft2(w) ** 2).mean(axis=(-2, -1))

    def compact(self, w):
        """rfft2-layout spectrum -> the solver's state layout [..., my1, nx] (kept y-wavenumbers, transposed)."""
        return np.swapaxes(w[..., :kept_y(self.ny)], -1, -2)


def taylor_green(nx, ny, t, nu, rho=1.0, Lx=2 * np.pi, Ly=2 * np.pi, U0=0.0, V0=0.0):
    """oracle/periodic.py: taylor_green translated by the mean flow: TG(x - U0 t, y - V0 t) + (U0, V0) (p unchanged in form)."""
    x = Lx * np.arange(nx) / nx - U0 * t
    y = Ly * np.arange(ny) / ny - V0 * t
    X, Y = np.meshgrid(x, y, indexing='ij')
    F = np.exp(-2 * nu * t)
    u = np.cos(X) * np.sin(Y) * F + U0
    v = -np.sin(X) * np.cos(Y) * F + V0
    p = -rho / 4. * (np.cos(2 * X) + np.cos(2 * Y)) * F * F
    return u, v, p


def random_ic(B, nx, ny, mmax, seed, Lx=2 * np.pi, Ly=2 * np.pi, umax=1.0, mean=(0.0, 0.0)):
    """Divergence-free velocity [B, nx, ny] from a random streamfunction with |m_x|, |m_y| <= mmax (amplitude ~ 1/|m|^2), scaled to
    max|u, v| = umax, plus a uniform mean."""
    rng = np.random.default_rng(seed)
    mx = np.fft.fftfreq(nx) * nx
    my = np.arange(ny // 2 + 1)
    band = (np.abs(mx)[:, None] <= mmax) & (my[None, :] <= mmax)
    band[0, 0] = False
    kx = (2 * np.pi / Lx * mx)[:, None]
    ky = (2 * np.pi / Ly * my)[None, :]
    mm = np.maximum(1.0, mx[:, None] ** 2 + my[None, :] ** 2)
    psi = (rng.standard_normal((B, nx, ny // 2 + 1)) + 1j * rng.standard_normal((B, nx, ny // 2 + 1))) * band / mm
    u = np.fft.irfft2(1j * ky * psi, s=(nx, ny))
    v = np.fft.irfft2(-1j * kx * psi, s=(nx, ny))
    s = umax / max(np.abs(u).max(), np.abs(v).max())
    return u * s + mean[0], v * s + mean[1]


def band_psi(B, nx, ny, seed):
    """Random streamfunction spectrum [B, nx, nh] over the whole 2/3 band (3|m_x| < nx, 3 m_y < ny, no (0, 0)), amplitude ~ 1/|m|^2 with
    m_x, m_y scaled to the shorter axis's band, Hermitian on the m_y = 0 column (psi(-m_x, 0) = conj psi(m_x, 0)): irfft2 then keeps
    every drawn coefficient."""
    rng = np.random.default_rng(seed)
    mx = np.fft.fftfreq(nx) * nx
    my = np.arange(ny // 2 + 1)
    Kx, Ky = (nx - 1) // 3, kept_y(ny) - 1
    K = min(Kx, Ky)                     # |m| with each axis rescaled to the shorter band: both edges are equally far out
    mm = (K * mx[:, None] / Kx) ** 2 + (K * my[None, :] / Ky) ** 2
    psi = (rng.standard_normal((B, nx, ny // 2 + 1)) + 1j * rng.standard_normal((B, nx, ny // 2 + 1))) * band(nx, ny) / np.maximum(1.0, mm)
    neg = (-np.arange(nx)) % nx
    psi[:, :, 0] = np.where((mx < 0)[None, :], np.conj(psi[:, neg, 0]), psi[:, :, 0])
    return psi


def band_ic(B, nx, ny, seed, Lx=2 * np.pi, Ly=2 * np.pi, umax=1.0, mean=(0.0, 0.0)):
    """Divergence-free velocity [B, nx, ny] whose spectrum fills the whole kept band (band_psi): energy reaches the edge modes of both
    axes, so the products of the nonlinear term spill past the band and alias.  Scaled to max|u, v| = umax, plus a uniform mean."""
    psi = band_psi(B, nx, ny, seed)
    mx = np.fft.fftfreq(nx) * nx
    my = np.arange(ny // 2 + 1)
    kx = (2 * np.pi / Lx * mx)[:, None]
    ky = (2 * np.pi / Ly * my)[None, :]
    u = np.fft.irfft2(1j * ky * psi, s=(nx, ny))
    v = np.fft.irfft2(-1j * kx * psi, s=(nx, ny))
    s = umax / max(np.abs(u).max(), np.abs(v).max())
    return u * s + mean[0], v * s + mean[1]


def cfl_dt(nx, ny, Lx, Ly, umax, cfl=0.5):
    """dt with dt umax (k_x,max + k_y,max) = cfl over the kept band: RK4 well inside its stability region."""
    kx = 2 * np.pi / Lx * ((nx - 1) // 3)
    ky = 2 * np.pi / Ly * (kept_y(ny) - 1)
    return cfl / (umax * (kx + ky))
