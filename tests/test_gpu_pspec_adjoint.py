"""GPU checks of the reverse mode of the periodic solver's step (csrc/pspec_kernels.hip: nns_spec_ns_step_adjoint_f32, ps_row_adj_kernel,
ps_col_adj_kernel; nns.periodic.PeriodicSolver.advance / advance_velocity) against the float64 restatement tests/pspec_adjoint_oracle.py,
analytic gradients and its own bit identities.  Inputs fill the whole 2/3 band (tests/pspec_adjoint_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_adjoint_cases as AC
import pspec_oracle as O

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = -1, -4
TWO_PI = 2 * np.pi


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def cplx(t):
    w = t.cpu().numpy().astype(np.float64)
    return w[..., 0] + 1j * w[..., 1]


def solver(c, dt, nu=AC.NU, drag=AC.DRAG, **kw):
    from nns.periodic import PeriodicSolver
    return PeriodicSolver(c[0], c[1], dt, AC.RHO, nu, Lx=c[3], Ly=c[4], drag=drag, **kw)


def forward(s, state, ghat, nsteps):
    """what0 [nsteps, B, my1, nx, 2] of nsteps forced steps of the state (advanced in place)."""
    from nns import ops
    what0 = torch.empty((nsteps,) + tuple(state.what.shape), dtype=torch.float32, device='cuda')
    for k in range(nsteps):
        what0[k].copy_(state.what)
        ops.spec_ns_step_forced_(state.what, state.mean, ghat, state.work, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, 1)
    return what0


def adjoint(s, what0, mean, ghat, lam, want_g=True, work=None):
    """(wbar, gbar) of the direct adjoint call; lam is not modified.  work: the workspace (None: a fresh one of the queried size)."""
    from nns import ops
    B = lam.shape[0]
    lam = lam.clone()
    gbar = torch.full_like(lam, float('nan')) if want_g else None            # overwritten, not added to
    if work is None:
        work = torch.empty(ops.spec_ns_adjoint_workspace(B, s.nx, s.ny), dtype=torch.uint8, device='cuda')
    ops.spec_ns_step_adjoint_(what0, mean, ghat, lam, gbar, work, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag)
    return lam, gbar


def direct(c, nsteps=AC.NSTEPS, grids=None):
    """(s, d, state0, ghat, lam, wbar, gbar) of the case through the C-level call; grids: a slice of the batch run alone."""
    d = AC.inputs(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = solver(c, d['dt'])
    ghat = s.init(dev(pick(d['fx'])), dev(pick(d['fy']))).what
    state = s.init(dev(pick(d['u0'])), dev(pick(d['v0'])))
    start = state.clone()
    lam = s.init_vorticity(dev(pick(d['r']))).what
    what0 = forward(s, state, ghat, nsteps)
    wbar, gbar = adjoint(s, what0, state.mean, ghat, lam)
    return s, d, start, ghat, lam, wbar, gbar


# ---------------------------------------------------------------------------------------------------- 1. against the float64 restatement
@pytest.mark.parametrize('case', AC.CASES, ids=AC.case_id)
def test_gradient_against_the_oracle(gpu_device, case):
    s, d, start, ghat, lam, wbar, gbar = direct(case)
    ref_w, ref_g = AC.oracle_gradient(case)
    ew, eg = AC.rel(cplx(wbar), ref_w), AC.rel(cplx(gbar), ref_g)
    print('MEASURED %s: wbar %.2e gbar %.2e' % (AC.case_id(case), ew, eg))
    assert ew <= AC.BOUND and eg <= AC.BOUND, (ew, eg)


# ---------------------------------------------------------------------------------------------------- 2. the autograd path
def test_advance_backward_is_the_direct_adjoint_call_bitwise(gpu_device):
    c = AC.CASES[0]
    d = AC.inputs(c)
    s = solver(c, d['dt'])
    st = s.init(dev(d['u0']), dev(d['v0']))
    w0 = s.vorticity(st).requires_grad_(True)
    mean = st.mean.clone()
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy'])))
    r = dev(d['r'])
    for forcing, reduce in ((g.clone().requires_grad_(True), False), (g[:1].clone().requires_grad_(True), True)):
        w0.grad = None
        out = s.advance(w0, AC.NSTEPS, mean=mean, forcing=forcing)
        (out * r).sum().backward()
        state = s.init_vorticity(w0.detach(), mean)
        ghat = s.init_vorticity(forcing.detach()).what
        same = s.init_vorticity(w0.detach(), mean)
        what0 = forward(s, state, ghat, AC.NSTEPS)
        assert torch.equal(out.detach(), s.vorticity(state))
        s.ghat = ghat                                                 # and the solver's own step with the same force
        s.step(same, AC.NSTEPS)
        s.ghat = None
        assert torch.equal(same.what, state.what)
        wbar, gbar = adjoint(s, what0, mean, ghat, s.init_vorticity(r).what)
        assert torch.equal(w0.grad, s.vorticity(state_of(wbar)))
        gf = s.vorticity(state_of(gbar))
        assert torch.equal(forcing.grad, torch.sum(gf, dim=0, keepdim=True) if reduce else gf)
        assert float(forcing.grad.abs().max()) > 0 and float(w0.grad.abs().max()) > 0


def test_advance_uses_the_solvers_force_as_a_constant(gpu_device):
    c = AC.CASES[0]
    d = AC.inputs(c)
    s = solver(c, d['dt'])
    st = s.init(dev(d['u0']), dev(d['v0']))
    w0 = s.vorticity(st)
    s.set_forcing(dev(d['fx'][:1]), dev(d['fy'][:1]))
    a = w0.clone().requires_grad_(True)
    out = s.advance(a, 2, mean=st.mean)
    same = s.init_vorticity(w0, st.mean)
    start = same.clone()
    s.step(same, 2)
    assert torch.equal(out.detach(), s.vorticity(same))
    r = dev(d['r'])
    (out * r).sum().backward()
    what0 = forward(s, start, s.ghat, 2)
    wbar, _ = adjoint(s, what0, st.mean, s.ghat, s.init_vorticity(r).what, want_g=False)
    assert torch.equal(a.grad, s.vorticity(state_of(wbar)))


def state_of(what):
    """A state at rest around a spectrum, to read it as a field."""
    from nns import ops
    from nns.periodic import PeriodicState
    B, my1, nx, _ = what.shape
    ny = {22: 64, 43: 128, 86: 256, 171: 512, 342: 1024}[my1]
    work = torch.empty(ops.spec_ns_scalar_workspace(B, nx, ny), dtype=torch.uint8, device='cuda')
    return PeriodicState(what, torch.zeros((B, 2), dtype=torch.float32, device='cuda'), work)


def test_advance_velocity_gradient_against_the_oracle(gpu_device):
    c = AC.CASES[0]
    nx, ny, B = c[:3]
    d = AC.inputs(c)
    s = solver(c, d['dt'])
    u0, v0 = dev(d['u0']).requires_grad_(True), dev(d['v0']).requires_grad_(True)
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    ru, rv = O.band_ic(B, nx, ny, 77, c[3], c[4], 1.0)
    ru, rv = ru.astype(np.float32), rv.astype(np.float32)
    u, v = s.advance_velocity(u0, v0, AC.NSTEPS, forcing=g)
    (u * dev(ru) + v * dev(rv)).sum().backward()
    st = s.init(u0.detach(), v0.detach())
    s.ghat = s.init_vorticity(g.detach()).what
    s.step(st, AC.NSTEPS)
    s.ghat = None
    fu, fv, _ = s.fields(st)
    assert torch.equal(u.detach(), fu) and torch.equal(v.detach(), fv)
    S = AC.scheme(c, d['dt'])
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    wbar, gbar = S.step_vjp(w, mean, S.velocity_vjp(ru.astype(np.float64), rv.astype(np.float64)), AC.NSTEPS)
    ub, vb = S.init_vjp(wbar)
    eu, ev = AC.rel(u0.grad.cpu().numpy().astype(np.float64), ub), AC.rel(v0.grad.cpu().numpy().astype(np.float64), vb)
    eg = AC.rel(g.grad.cpu().numpy().astype(np.float64), S.irfft2(gbar))
    print('MEASURED advance_velocity %s: u0 %.2e v0 %.2e g %.2e' % (AC.case_id(c), eu, ev, eg))
    assert max(eu, ev, eg) <= AC.BOUND, (eu, ev, eg)


# ---------------------------------------------------------------------------------------------------- 3. analytic checks
def test_gradient_from_rest_is_the_decayed_projected_cotangent(gpu_device):
    c = (64, 128, 2, 3.0, 7.0, (0.0, 0.0))
    s = solver(c, 0.01, nu=1e-2, drag=0.3)
    rng = np.random.default_rng(3)
    mu = rng.standard_normal((2, 64, 128)).astype(np.float32)              # white: content outside the band and a mean
    w0 = torch.zeros((2, 64, 128), device='cuda', requires_grad=True)
    out = s.advance(w0, 3)
    assert float(out.detach().abs().max()) == 0.0
    (out * dev(mu)).sum().backward()
    S = AC.scheme(c, 0.01)
    ref = S.irfft2(np.exp(-(1e-2 * S.k2 + 0.3) * 0.01 * 3) * S.M * np.fft.rfft2(mu.astype(np.float64)))
    err = AC.rel(w0.grad.cpu().numpy().astype(np.float64), ref)
    print('from rest: rel %.2e' % err)
    assert err <= 2e-6


def test_cotangent_outside_the_band_contributes_nothing(gpu_device):
    c = AC.CASES[0]
    nx, ny, B = c[:3]
    s, d, start, ghat, lam, wbar, gbar = direct(c)
    S = AC.scheme(c, d['dt'])
    rng = np.random.default_rng(4)
    outside = np.fft.irfft2((1 - S.M) * np.fft.rfft2(rng.standard_normal((B, nx, ny))), s=(nx, ny))     # the (0, 0) mode and everything beyond the band
    outside *= np.sqrt((d['r'].astype(np.float64) ** 2).mean() / (outside ** 2).mean())                 # as large as r
    w0 = s.vorticity(start)
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy'])))
    grads = []
    for r in (d['r'], d['r'] + outside.astype(np.float32)):
        a, f = w0.clone().requires_grad_(True), g.clone().requires_grad_(True)
        (s.advance(a, AC.NSTEPS, mean=start.mean, forcing=f) * dev(r)).sum().backward()
        grads.append((a.grad, f.grad))
    # the compact kernel drops the rest exactly; what remains is the float32 rounding of rfft2 on an input of twice the energy:
    # eps log2(nx ny) (1 + 1) = 6e-8 x 12 x 2 = 1.5e-6, rounded up
    for x, y in zip(grads[0], grads[1]):
        assert float((x - y).norm() / x.norm()) <= 2e-6
    for t in (wbar, gbar):                                                # zero mean, nothing outside the band
        z = cplx(t)
        keep = S.compact(S.M).real > 0
        assert np.all(z[:, ~keep] == 0) and np.all(np.abs(z[:, keep]).max() > 0)


# ---------------------------------------------------------------------------------------------------- 4. bit identities
@pytest.mark.parametrize('case', [AC.CASES[0], AC.CASES[4]], ids=AC.case_id)
def test_a_batch_is_its_grids_and_one_call_is_chained_calls(gpu_device, case):
    s, d, start, ghat, lam, wbar, gbar = direct(case)
    B = case[2]
    for b in range(B):
        _, _, _, _, _, w1, g1 = direct(case, grids=slice(b, b + 1))
        assert torch.equal(w1[0], wbar[b]) and torch.equal(g1[0], gbar[b])
    state = start.clone()
    what0 = forward(s, state, ghat, AC.NSTEPS)
    l, gsum = lam, None
    for k in reversed(range(AC.NSTEPS)):
        l, g = adjoint(s, what0[k:k + 1], start.mean, ghat, l)
        gsum = g if gsum is None else gsum + g
    assert torch.equal(l, wbar)
    assert float((gsum - gbar).abs().max()) <= 1e-6 * float(gbar.abs().max())     # the call sums in another order: stage by stage
    lw, none = adjoint(s, what0, start.mean, ghat, lam, want_g=False)
    assert none is None and torch.equal(lw, wbar)


def test_grid_stride(gpu_device):
    c = AC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = AC.C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    r = O.band_ic(4, nx, ny, 5, c[3], c[4], 1.0)[0]
    s = solver(c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]))
        lam = s.init_vorticity(dev(r[sel])).what
        what0 = forward(s, state, None, 1)
        outs.append(adjoint(s, what0, state.mean, None, lam))
    (wb, gb), (w01, g01), (w23, g23) = outs
    assert torch.equal(wb[:2], w01) and torch.equal(gb[:2], g01) and torch.equal(wb[-2:], w23) and torch.equal(gb[-2:], g23)
    assert float(wb.abs().max()) > 0


def test_the_call_stays_inside_its_workspace(gpu_device):
    """64 x 64 (the smallest grid on both axes: 22 kept columns in one 64-line tile), one grid, 2 steps, gbar wanted: the bytes after the
    queried size keep their fill, and the results are those of a plain workspace of that size."""
    from nns import ops
    s, d, start, ghat, lam, wbar, gbar = direct(AC.CASES[0], nsteps=2, grids=slice(0, 1))
    what0 = forward(s, start.clone(), ghat, 2)
    need = ops.spec_ns_adjoint_workspace(1, s.nx, s.ny)
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    w2, g2 = adjoint(s, what0, start.mean, ghat, lam, work=buf[:need])
    assert bool((buf[need:] == 0xA5).all())
    assert torch.equal(w2, wbar) and torch.equal(g2, gbar) and float(gbar.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize('kw,name', [(dict(kappa=1e-3), 'kappa'), (dict(kappa=1e-3, buoyancy=(0.0, 1.0)), 'buoyancy'),
                                     (dict(hyperviscosity=(1e-8, 2)), 'hyperviscosity'), (dict(hypofriction=(0.1, 1)), 'hypofriction'),
                                     (dict(beta=1.0), 'beta'), (dict(), 'set_stochastic_forcing')])
def test_unsupported_solvers_are_refused(gpu_device, kw, name):
    s = solver((64, 64, 1, TWO_PI, TWO_PI), 0.01, **kw)
    if name == 'set_stochastic_forcing':
        s.ring_forcing(1.0, 3.0, 5.0)
    w = torch.zeros((1, 64, 64), device='cuda', requires_grad=True)
    for call in (lambda: s.advance(w, 1), lambda: s.advance_velocity(w, w, 1)):
        with pytest.raises(NotImplementedError, match=name):
            call()


def test_bad_tensors_are_refused(gpu_device):
    s = solver((64, 64, 1, TWO_PI, TWO_PI), 0.01)
    ok = torch.zeros((1, 64, 64), device='cuda')
    with pytest.raises(TypeError):
        s.advance(torch.zeros(1, 64, 64), 1)
    with pytest.raises(TypeError):
        s.advance(ok.double(), 1)
    with pytest.raises(TypeError):
        s.advance(ok, 1, forcing=torch.zeros(1, 64, 64))
    with pytest.raises(ValueError):
        s.advance(torch.zeros((1, 64, 128), device='cuda'), 1)
    with pytest.raises(ValueError):
        s.advance(ok, 1, forcing=torch.zeros((3, 64, 64), device='cuda'))
    with pytest.raises(ValueError):
        s.advance(ok, 0)
    with pytest.raises(ValueError):
        s.advance_velocity(ok, torch.zeros((2, 64, 64), device='cuda'), 1)
    with pytest.raises(TypeError):
        s.advance_velocity(ok, ok.cpu(), 1)


def test_c_entry_points_refuse_null_and_a_short_workspace(gpu_device):
    from nns import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    from nns import ops
    assert L.nns_spec_ns_adjoint_workspace(2, 64, 64, ctypes.byref(n)) == 0
    assert n.value == max(13 * 2 * 64 * 22 * 8, ops.spec_ns_workspace(2, 64, 64))          # 13 compacted fields, and it serves the forward calls
    assert L.nns_spec_ns_adjoint_workspace(2, 64, 64, None) == INVALID
    t = torch.zeros(n.value, dtype=torch.uint8, device='cuda')
    P = t.data_ptr()
    args = lambda what0=P, lam=P, work=P, nbytes=n.value: (what0, P, None, 0, lam, None, work, nbytes, 2, 64, 64, TWO_PI, TWO_PI, 0.01, 1e-3, 0.0, 1, None)
    assert L.nns_spec_ns_step_adjoint_f32(*args(what0=None)) == INVALID
    assert L.nns_spec_ns_step_adjoint_f32(*args(lam=None)) == INVALID
    assert L.nns_spec_ns_step_adjoint_f32(*args(work=None)) == INVALID
    assert L.nns_spec_ns_step_adjoint_f32(*args(nbytes=n.value - 1)) == WORKSPACE
    assert b'nns_spec_ns_adjoint_workspace' in L.nns_last_error()
