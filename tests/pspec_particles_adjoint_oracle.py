"""NumPy float64 restatement (tests only) of the reverse mode of the periodic solver's particle sampling (csrc/pspec_particles.hip:
nns_spec_ns_particle_cells_i32, _spread_f32, _sample_grad_f32, _coefs_adjoint_f32; nns.periodic.PeriodicSolver.observe / spread /
sample_gradient / particle_cells).  It builds on tests/pspec_particles_oracle.py by import only.

(a) spread(r, x, y, ...): the transpose of pspec_particles_oracle.evaluate, image[i0 + a, j0 + c] += wx[a] wy[c] r (indices modulo the axis).
(b) gradient(c, x, y, ...): (d/dx, d/dy) of the spline, (1 / hx) sum_a wx'[a] (sum_c wy[c] C) and (1 / hy) sum_a wx[a] (sum_c wy'[c] C), with
    dweights(t, order) the derivative of pspec_particles_oracle.weights in t.
(c) build(w, theta, mean, ...): the coefficient images of u, v, w, theta of the FIELDS w and theta as the solver makes them
        W = M rfft2(w), W(0, 0) = 0;  u^ = i ky W / |k|^2, v^ = -i kx W / |k|^2, their (0, 0) modes the mean flow;  T = M rfft2(theta);
        c = irfft2(f^ / (beta_x beta_y))       (M: the 2/3 band, 3 |m_x| < nx and 3 m_y < ny)
    and build_adjoint(cbar, ...), its transpose between physical fields: with c^ = rfft2(cbar),
        wbar = irfft2( M [(-i ky c_u^ + i kx c_v^) / |k|^2 + c_w^] / (beta_x beta_y) ), (0, 0) zero;   thetabar = irfft2( M c_theta^ / (beta_x beta_y) ).
    The map is real, so the transpose takes the conjugate multipliers and no half-spectrum weights arise.
(d) observe(...) and observe_gradients(...): the values at the points and the gradients of sum(values . r) in w, theta, x and y.
(e) WRONG: deliberately wrong variants (mutation tests) -- 'no_beta': the transpose without the division by beta; 'unconjugated': the
    forward's multipliers where their conjugates belong; 'swapped': the x and y weights exchanged in the spread and the gradient;
    'dweight_sign': the sign of the t^2 term of a derivative weight flipped (order 4: node 1, +3t^2 -> -3t^2; order 6: the 450 x^2 term of
    the middle piece); 'no_h': the gradient without its 1 / h.
"""
import numpy as np

import pspec_particles_oracle as PO

WRONG = ('no_beta', 'unconjugated', 'swapped', 'dweight_sign', 'no_h')
FIELDS = ('u', 'v', 'w', 'theta')


def dweights(t, order, wrong=None):
    """[order, ...]: d/dt of pspec_particles_oracle.weights(t, order)."""
    t = np.asarray(t, dtype=np.float64)
    flip = -1.0 if wrong == 'dweight_sign' else 1.0
    if order == 4:
        return np.stack([-(1.0 - t) ** 2 / 2.0, (flip * 3.0 * t ** 2 - 4.0 * t) / 2.0, (-3.0 * t ** 2 + 2.0 * t + 1.0) / 2.0, t ** 2 / 2.0])
    inner = lambda x: (-120.0 * x + 120.0 * x ** 3 - 50.0 * x ** 4) / 120.0
    middle = lambda x: (75.0 - 420.0 * x + flip * 450.0 * x ** 2 - 180.0 * x ** 3 + 25.0 * x ** 4) / 120.0
    outer = lambda r: r ** 4 / 24.0
    return np.stack([-outer(1.0 - t), middle(t + 1.0), inner(t), -inner(1.0 - t), -middle(2.0 - t), outer(t)])


def locate(x, h, n, order):
    """(first node, offset, cell) of the coordinates x on an axis of n nodes of spacing h, as the kernel takes them."""
    s = np.asarray(x, dtype=np.float64) / h
    fl = np.floor(s)
    cell = np.mod(fl, n).astype(np.int64) % n
    return (cell - (order // 2 - 1)) % n, s - fl, cell


def cell_keys(x, y, nx, ny, Lx, Ly):
    """int64 [B, P]: (b nx + ci) ny + cj of the points x, y [B, P]."""
    ci, cj = locate(x, Lx / nx, nx, 4)[2], locate(y, Ly / ny, ny, 4)[2]
    return (np.arange(x.shape[0])[:, None] * nx + ci) * ny + cj


def spread(r, x, y, nx, ny, Lx, Ly, order, wrong=None):
    """[B, nx, ny]: the transpose of the gather applied to r [B, P] at the points x, y [B, P]."""
    i0, tx, _ = locate(x, Lx / nx, nx, order)
    j0, ty, _ = locate(y, Ly / ny, ny, order)
    wx, wy = PO.weights(tx, order), PO.weights(ty, order)
    if wrong == 'swapped':
        wx, wy = wy, wx
    out = np.zeros((x.shape[0], nx, ny))
    b = np.broadcast_to(np.arange(x.shape[0])[:, None], x.shape)
    for a in range(order):
        for c in range(order):
            np.add.at(out, (b, (i0 + a) % nx, (j0 + c) % ny), wx[a] * wy[c] * r)
    return out


def gradient(c, x, y, Lx, Ly, order, wrong=None):
    """[B, P, 2]: (d/dx, d/dy) of the spline of the coefficients c [B, nx, ny] at the points x, y [B, P]."""
    nx, ny = c.shape[-2:]
    hx, hy = Lx / nx, Ly / ny
    i0, tx, _ = locate(x, hx, nx, order)
    j0, ty, _ = locate(y, hy, ny, order)
    wx, wy, dwx, dwy = PO.weights(tx, order), PO.weights(ty, order), dweights(tx, order, wrong), dweights(ty, order, wrong)
    if wrong == 'swapped':
        wx, wy, dwx, dwy = wy, wx, dwy, dwx
    b = np.broadcast_to(np.arange(x.shape[0])[:, None], x.shape)
    gx, gy = np.zeros(x.shape), np.zeros(x.shape)
    for a in range(order):
        row, rowd = np.zeros(x.shape), np.zeros(x.shape)
        for k in range(order):
            v = c[b, (i0 + a) % nx, (j0 + k) % ny]
            row += wy[k] * v
            rowd += dwy[k] * v
        gx += dwx[a] * row
        gy += wx[a] * rowd
    if wrong != 'no_h':
        gx, gy = gx / hx, gy / hy
    return np.stack([gx, gy], axis=-1)


def _tables(nx, ny, Lx, Ly, order):
    """(band mask, kx, ky, 1 / |k|^2 with 0 at (0, 0), beta_x beta_y), each [nx, nh]."""
    mx, my = np.fft.fftfreq(nx) * nx, np.arange(ny // 2 + 1)
    band = ((3 * np.abs(mx) < nx)[:, None] & (3 * my < ny)[None, :]).astype(np.float64)
    kx, ky = np.broadcast_arrays((2 * np.pi / Lx * mx)[:, None], (2 * np.pi / Ly * my)[None, :])
    k2 = kx ** 2 + ky ** 2
    ik2 = np.where(k2 > 0, 1.0 / np.where(k2 > 0, k2, 1.0), 0.0)
    bb = PO.beta(2 * np.pi * mx / nx, order)[:, None] * PO.beta(2 * np.pi * my / ny, order)[None, :]
    return band, kx, ky, ik2, bb


def build(w, theta, mean, Lx, Ly, order):
    """dict by field name of the coefficient images [B, nx, ny] of the fields w (and theta, or None) [B, nx, ny] with the mean flow
    mean [B, 2] (or None: at rest).  Linear in (w, theta) for mean None."""
    w = np.asarray(w, dtype=np.float64)
    nx, ny = w.shape[-2:]
    band, kx, ky, ik2, bb = _tables(nx, ny, Lx, Ly, order)
    W = band * np.fft.rfft2(w)
    W[..., 0, 0] = 0.0
    uh, vh = 1j * ky * ik2 * W, -1j * kx * ik2 * W
    if mean is not None:
        uh[..., 0, 0], vh[..., 0, 0] = np.asarray(mean)[:, 0] * nx * ny, np.asarray(mean)[:, 1] * nx * ny
    sp = dict(u=uh, v=vh, w=W)
    if theta is not None:
        sp['theta'] = band * np.fft.rfft2(np.asarray(theta, dtype=np.float64))
    return {f: np.fft.irfft2(s / bb, s=(nx, ny)) for f, s in sp.items()}


def build_adjoint(cbar, Lx, Ly, order, wrong=None):
    """(wbar, thetabar), fields [B, nx, ny] (None where cbar names none of u, v, w / no theta): the transpose of ``build`` applied to the
    dict cbar of cotangent images by field name."""
    first = next(iter(cbar.values()))
    nx, ny = first.shape[-2:]
    band, kx, ky, ik2, bb = _tables(nx, ny, Lx, Ly, order)
    if wrong == 'no_beta':
        bb = np.ones_like(bb)
    sign = -1.0 if wrong == 'unconjugated' else 1.0
    ch = {f: np.fft.rfft2(np.asarray(c, dtype=np.float64)) for f, c in cbar.items()}
    wbar = thbar = None
    if any(f in ch for f in ('u', 'v', 'w')):
        acc = np.zeros_like(next(iter(ch.values())))
        if 'u' in ch:
            acc = acc - sign * 1j * ky * ik2 * ch['u']
        if 'v' in ch:
            acc = acc + sign * 1j * kx * ik2 * ch['v']
        if 'w' in ch:
            acc = acc + ch['w']
        acc = band * acc / bb
        acc[..., 0, 0] = 0.0
        wbar = np.fft.irfft2(acc, s=(nx, ny))
    if 'theta' in ch:
        thbar = np.fft.irfft2(band * ch['theta'] / bb, s=(nx, ny))
    return wbar, thbar


def _points(x, y, B):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return (np.broadcast_to(x, (B,) + x.shape[-1:]), np.broadcast_to(y, (B,) + y.shape[-1:]))


def observe(w, theta, mean, x, y, fields, Lx, Ly, order):
    """[B, P, len(fields)]: ``fields`` of (w, theta, mean) at the points x, y ([B, P], or [P] shared by the B grids)."""
    coef = build(w, theta, mean, Lx, Ly, order)
    x, y = _points(x, y, np.shape(w)[0])
    return np.stack([PO.evaluate(coef[f], x, y, Lx, Ly, order) for f in fields], axis=-1)


def observe_gradients(w, theta, mean, x, y, fields, r, Lx, Ly, order, wrong=None):
    """(wbar, thetabar, xbar, ybar): the gradients of sum(observe(...) . r), r [B, P, len(fields)]; xbar, ybar shaped like x, y (summed over
    the grids for shared points)."""
    w = np.asarray(w, dtype=np.float64)
    B, nx, ny = w.shape
    shared = np.ndim(x) == 1
    X, Y = _points(x, y, B)
    r = np.asarray(r, dtype=np.float64)
    cbar = {}
    for k, f in enumerate(fields):
        cbar[f] = cbar.get(f, 0.0) + spread(r[..., k], X, Y, nx, ny, Lx, Ly, order, wrong)
    wbar, thbar = build_adjoint(cbar, Lx, Ly, order, wrong)
    coef = build(w, theta, mean, Lx, Ly, order)
    pbar = sum(r[..., k, None] * gradient(coef[f], X, Y, Lx, Ly, order, wrong) for k, f in enumerate(fields))
    if shared:
        pbar = pbar.sum(axis=0)
    return wbar, thbar, pbar[..., 0], pbar[..., 1]
