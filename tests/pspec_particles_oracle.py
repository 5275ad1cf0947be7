"""NumPy float64 restatement (tests only) of the Lagrangian tracers of the periodic solver (csrc/pspec_particles.hip: nns_spec_ns_particle_*;
nns.periodic.PeriodicSolver.init_particles / particle_coefficients / sample / advect).

(a) exact(fh, x, y): a band-limited field at arbitrary points by the direct Fourier sum over its stored modes,
        f(x, y) = 1/n sum_(m_x, m_y >= 0) wt Re( f^(m_x, m_y) exp(i (kx x + ky y)) ),   wt = 1 on m_y = 0, 2 on m_y > 0.
(b) Periodic tensor-product B-splines of order 4 (cubic) or 6 (quintic) with the exact prefilter:
        c = irfft2( f^ / (beta(2 pi m_x / nx) beta(2 pi m_y / ny)) ),   beta(t) = (2 + cos t) / 3   or   (66 + 52 cos t + 2 cos 2t) / 120;
    a point x has cell i = floor(x / hx) and offset t = x / hx - i, nodes i-1 .. i+2 (i-2 .. i+3) modulo n, weights of weights(t, order).
    The fields: u, v (the mean flow in the (0, 0) coefficient), w, theta, from the flow restatement's spectra (tests/pspec_oracle.py: Scheme
    and its children; this file drives them and edits none).
(c) Tracers: positions unwrapped; classical RK4 of step H = 2 dt over a pair of flow steps,
        k1 = U_n(x);  k2 = U_n+1(x + dt k1);  k3 = U_n+1(x + dt k2);  k4 = U_n+2(x + 2 dt k3);  x <- x + dt/3 (k1 + 2 k2 + 2 k3 + k4),
    U the spline (or, sampler='exact', the Fourier sum) of the flow at the step boundaries; Heun over one step,
        x* = x + dt U_n(x);  x <- x + dt/2 (U_n(x) + U_n+1(x*)).
(d) WRONG: deliberately wrong variants (mutation tests) -- 'shifted': the stencil one node to the right; 'swapped': the x and y weights exchanged;
    'unfiltered': no prefilter (the samples taken as coefficients); 'no_mean': the mean flow left out; 'stale': U_n in stages 2-3 of RK4 (and
    in Heun's corrector); 'half_step': the closing weights of a step H = dt (dt/6 for RK4, dt/4 for Heun).
"""
import numpy as np

WRONG = ('shifted', 'swapped', 'unfiltered', 'no_mean', 'stale', 'half_step')
SAMPLING = ('shifted', 'swapped', 'unfiltered', 'no_mean')           # those that a single read of the flow shows


def beta(theta, order):
    if order == 4:
        return (2.0 + np.cos(theta)) / 3.0
    return (66.0 + 52.0 * np.cos(theta) + 2.0 * np.cos(2.0 * theta)) / 120.0


def b5(x):
    """The centred quintic B-spline."""
    x = np.abs(x)
    inner = (66.0 - 60.0 * x ** 2 + 30.0 * x ** 4 - 10.0 * x ** 5) / 120.0
    middle = (51.0 + 75.0 * x - 210.0 * x ** 2 + 150.0 * x ** 3 - 45.0 * x ** 4 + 5.0 * x ** 5) / 120.0
    outer = np.where(x < 3.0, 3.0 - x, 0.0) ** 5 / 120.0
    return np.where(x < 1.0, inner, np.where(x < 2.0, middle, outer))


def weights(t, order):
    """[order, ...]: the weights of the nodes i - (order / 2 - 1) ... at offset t."""
    t = np.asarray(t, dtype=np.float64)
    if order == 4:
        return np.stack([(1.0 - t) ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0,
                         (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0, t ** 3 / 6.0])
    return np.stack([b5(t - j) for j in range(-2, 4)])


def exact(fh, x, y, nx, ny, Lx, Ly):
    """fh [..., nx, nh] (rfft2 layout, unnormalised) at the points x, y [..., P] (leading axes those of fh): the Fourier sum, [..., P]."""
    fh = np.asarray(fh)
    lead = fh.shape[:-2]
    x, y = np.broadcast_to(x, lead + np.shape(x)[-1:]), np.broadcast_to(y, lead + np.shape(y)[-1:])
    mx = np.fft.fftfreq(nx) * nx
    out = np.zeros(x.shape)
    for idx in np.ndindex(*lead):
        f = fh[idx]
        ii, jj = np.nonzero(f)
        wt = np.where((jj == 0) | (2 * jj == ny), 1.0, 2.0)
        ph = np.exp(1j * (np.outer(x[idx], 2 * np.pi / Lx * mx[ii]) + np.outer(y[idx], 2 * np.pi / Ly * jj)))
        out[idx] = (ph * (wt * f[ii, jj])).real.sum(axis=1) / (nx * ny)
    return out


def coefficients(fh, nx, ny, order, wrong=None):
    """The spline coefficients [..., nx, ny] of the field of spectrum fh [..., nx, nh]."""
    if wrong == 'unfiltered':
        return np.fft.irfft2(fh, s=(nx, ny))
    bx = beta(2 * np.pi * np.fft.fftfreq(nx), order)[:, None]
    by = beta(2 * np.pi * np.arange(ny // 2 + 1) / ny, order)[None, :]
    return np.fft.irfft2(fh / (bx * by), s=(nx, ny))


def evaluate(c, x, y, Lx, Ly, order, wrong=None):
    """The spline of coefficients c [..., nx, ny] at the points x, y [..., P]: [..., P].  Cell and offset as the kernel takes them: float64
    x / h, its floor, the difference."""
    nx, ny = c.shape[-2:]
    lead = c.shape[:-2]
    x, y = np.broadcast_to(x, lead + np.shape(x)[-1:]), np.broadcast_to(y, lead + np.shape(y)[-1:])
    sx, sy = x / (Lx / nx), y / (Ly / ny)
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = weights(sx - fx, order), weights(sy - fy, order)
    if wrong == 'swapped':
        wx, wy = wy, wx
    first = order // 2 - 1 - (1 if wrong == 'shifted' else 0)
    i0 = (np.mod(fx, nx).astype(np.int64) - first) % nx
    j0 = (np.mod(fy, ny).astype(np.int64) - first) % ny
    out = np.zeros(x.shape)
    for idx in np.ndindex(*lead):
        cc = c[idx]
        for a in range(order):
            row = np.zeros(x.shape[-1])
            for b in range(order):
                row += wy[(b,) + idx] * cc[(i0[idx] + a) % nx, (j0[idx] + b) % ny]
            out[idx] += wx[(a,) + idx] * row
    return out


class Tracers(object):
    """Tracers in the flow of ``flow`` (a tests/pspec_oracle.py Scheme or a child: LinearScheme serves every solver).  order: 4 or 6; sampler:
    'spline' or 'exact'; wrong: None or one of WRONG."""

    def __init__(self, flow, order=4, sampler='spline', wrong=None):
        if wrong is not None and wrong not in WRONG:
            raise ValueError("wrong must be None or one of %s" % (WRONG,))
        if sampler not in ('spline', 'exact'):
            raise ValueError("sampler must be 'spline' or 'exact'")
        self.flow, self.order, self.sampler, self.wrong = flow, order, sampler, wrong

    def spectra(self, w, mean, t=None):
        """dict of the spectra of u, v, w (and theta) of a state."""
        F = self.flow
        uh, vh = F.velocity_hat(w, mean)
        if self.wrong == 'no_mean':
            uh[..., 0, 0] = 0.0
            vh[..., 0, 0] = 0.0
        out = dict(u=uh, v=vh, w=w)
        if t is not None:
            out['theta'] = t
        return out

    def coefficients(self, w, mean, t=None, fields=('u', 'v')):
        F, sp = self.flow, self.spectra(w, mean, t)
        return tuple(coefficients(sp[f], F.nx, F.ny, self.order, self.wrong) for f in fields)

    def sample(self, w, mean, pos, t=None, fields=('u', 'v')):
        """[..., P, len(fields)] at pos [..., P, 2]."""
        F, sp = self.flow, self.spectra(w, mean, t)
        x, y = pos[..., 0], pos[..., 1]
        if self.sampler == 'exact':
            vals = [exact(sp[f], x, y, F.nx, F.ny, F.Lx, F.Ly) for f in fields]
        else:
            vals = [evaluate(coefficients(sp[f], F.nx, F.ny, self.order, self.wrong), x, y, F.Lx, F.Ly, self.order, self.wrong) for f in fields]
        return np.stack(vals, axis=-1)

    def _flow_step(self, w, mean, t):
        return (self.flow.step(w, mean, 1), None) if t is None else self.flow.step(w, t, mean, 1)

    def advect(self, w, mean, pos, nsteps, scheme='rk4', t=None):
        """(w, t, pos) after nsteps steps of the flow and of the particles pos [..., P, 2] in it."""
        if scheme == 'rk4' and nsteps % 2:
            raise ValueError("rk4 advances over pairs of flow steps")
        dt, stale, half = self.flow.dt, self.wrong == 'stale', self.wrong == 'half_step'
        U = lambda w_, p: self.sample(w_, mean, p)
        pos = np.array(pos, dtype=np.float64)
        if scheme == 'rk4':
            for _ in range(nsteps // 2):
                w1, t1 = self._flow_step(w, mean, t)
                w2, t2 = self._flow_step(w1, mean, t1)
                mid = w if stale else w1
                k1 = U(w, pos)
                k2 = U(mid, pos + dt * k1)
                k3 = U(mid, pos + dt * k2)
                k4 = U(w2, pos + 2 * dt * k3)
                pos = pos + (dt / 6 if half else dt / 3) * (k1 + 2 * k2 + 2 * k3 + k4)
                w, t = w2, t2
        else:
            for _ in range(nsteps):
                w1, t1 = self._flow_step(w, mean, t)
                k1 = U(w, pos)
                k2 = U(w if stale else w1, pos + dt * k1)
                pos = pos + (dt / 4 if half else dt / 2) * (k1 + k2)
                w, t = w1, t1
        return w, t, pos
