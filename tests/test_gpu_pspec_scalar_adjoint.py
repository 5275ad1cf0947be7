"""GPU checks of the reverse mode of the periodic solver's scalar and buoyant step (csrc/pspec_kernels.hip:
nns_spec_ns_step_scalar_adjoint_f32, ps_row_adj_kernel and ps_col_adj_kernel in their scalar forms; nns.periodic.PeriodicSolver.advance_scalar /
advance_velocity_scalar) against the float64 restatement tests/pspec_scalar_adjoint_oracle.py, the flow's own adjoint, an analytic gradient and
its own bit identities.  Inputs fill the whole 2/3 band (tests/pspec_scalar_adjoint_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_oracle as O
import pspec_scalar_adjoint_cases as AC

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = -1, -4
TWO_PI = 2 * np.pi


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def cplx(t):
    w = t.cpu().numpy().astype(np.float64)
    return w[..., 0] + 1j * w[..., 1]


def solver(c, dt, nu=AC.NU, drag=AC.DRAG, kappa=AC.KAPPA, grad=AC.GRAD, **kw):
    from nns.periodic import PeriodicSolver
    return PeriodicSolver(c[0], c[1], dt, AC.RHO, nu, Lx=c[3], Ly=c[4], drag=drag, kappa=kappa, scalar_gradient=grad, buoyancy=c[6], **kw)


def forward(s, state, ghat, nsteps):
    """(what0, that0) [nsteps, B, my1, nx, 2] of nsteps steps of the state (advanced in place): the buoyant step with b != 0, else the scalar's."""
    from nns import ops
    what0 = torch.empty((nsteps,) + tuple(state.what.shape), dtype=torch.float32, device='cuda')
    that0 = torch.empty_like(what0)
    box = (state.mean, ghat, state.work, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient)
    for k in range(nsteps):
        what0[k].copy_(state.what)
        that0[k].copy_(state.that)
        if s.buoyancy != (0.0, 0.0):
            ops.spec_ns_step_buoyant_(state.what, state.that, *box, s.buoyancy, 1)
        else:
            ops.spec_ns_step_scalar_(state.what, state.that, *box, 1)
    return what0, that0


def adjoint(s, what0, that0, mean, ghat, lam, mu, want_g=True, work=None):
    """(wbar, thetabar, gbar) of the direct adjoint call; lam and mu are not modified.  work: the workspace (None: a fresh one of the queried
    size)."""
    from nns import ops
    B = lam.shape[0]
    lam, mu = lam.clone(), mu.clone()
    gbar = torch.full_like(lam, float('nan')) if want_g else None            # overwritten, not added to
    if work is None:
        work = torch.empty(ops.spec_ns_scalar_adjoint_workspace(B, s.nx, s.ny), dtype=torch.uint8, device='cuda')
    ops.spec_ns_step_scalar_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa,
                                     s.scalar_gradient, s.buoyancy)
    return lam, mu, gbar


def scalar_spectrum(s, field):
    """M_theta rfft2 of a field [B, nx, ny] in the state's layout: the scalar's compact kernel."""
    return s.init(torch.zeros_like(field), torch.zeros_like(field), field).that


def direct(c, nsteps=AC.NSTEPS, grids=None):
    """(s, d, state0, ghat, lam, mu, wbar, thetabar, gbar) of the case through the C-level call; grids: a slice of the batch run alone."""
    d = AC.inputs(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = solver(c, d['dt'])
    ghat = s.init(dev(pick(d['fx'])), dev(pick(d['fy']))).what
    state = s.init(dev(pick(d['u0'])), dev(pick(d['v0'])), dev(pick(d['theta0'])))
    start = state.clone()
    lam = s.init_vorticity(dev(pick(d['rw']))).what
    mu = scalar_spectrum(s, dev(pick(d['rt'])))
    what0, that0 = forward(s, state, ghat, nsteps)
    return (s, d, start, ghat, lam, mu) + adjoint(s, what0, that0, state.mean, ghat, lam, mu)


def state_of(s, what):
    """A state at rest around a spectrum of the solver s, to read it as a field."""
    from nns import ops
    from nns.periodic import PeriodicState
    B = what.shape[0]
    work = torch.empty(ops.spec_ns_scalar_workspace(B, s.nx, s.ny), dtype=torch.uint8, device='cuda')
    return PeriodicState(what, torch.zeros((B, 2), dtype=torch.float32, device='cuda'), work)


def field_of(s, that):
    """The field of a scalar spectrum of the solver s."""
    from nns import ops
    return ops.spec_ns_scalar_field(that, state_of(s, that).work, s.ny)


# ---------------------------------------------------------------------------------------------------- 1. against the float64 restatement
@pytest.mark.parametrize('case', AC.CASES, ids=AC.case_id)
def test_gradient_against_the_oracle(gpu_device, case):
    s, d, start, ghat, lam, mu, wbar, tbar, gbar = direct(case)
    errs = tuple(AC.rel(cplx(g), r) for g, r in zip((wbar, tbar, gbar), AC.oracle_gradient(case)))
    print('MEASURED %s: wbar %.2e thetabar %.2e gbar %.2e' % ((AC.case_id(case),) + errs))
    assert max(errs) <= AC.BOUND, errs


# ---------------------------------------------------------------------------------------------------- 2. the autograd path
@pytest.mark.parametrize('case', AC.CASES[:2], ids=AC.case_id)
def test_advance_scalar_backward_is_the_direct_adjoint_call_bitwise(gpu_device, case):
    c = case
    d = AC.inputs(c)
    s = solver(c, d['dt'])
    st = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']))
    w0 = s.vorticity(st).requires_grad_(True)
    th0 = dev(d['theta0']).requires_grad_(True)
    mean = st.mean.clone()
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy'])))
    rw, rt = dev(d['rw']), dev(d['rt'])
    for forcing, reduce in ((g.clone().requires_grad_(True), False), (g[:1].clone().requires_grad_(True), True)):
        w0.grad = th0.grad = None
        ow, ot = s.advance_scalar(w0, th0, AC.NSTEPS, mean=mean, forcing=forcing)
        ((ow * rw).sum() + (ot * rt).sum()).backward()
        state = s.init_vorticity(w0.detach(), mean)
        state.that = scalar_spectrum(s, th0.detach())
        same = state.clone()
        ghat = s.init_vorticity(forcing.detach()).what
        what0, that0 = forward(s, state, ghat, AC.NSTEPS)
        assert torch.equal(ow.detach(), s.vorticity(state)) and torch.equal(ot.detach(), s.scalar(state))
        s.ghat = ghat                                                 # and the solver's own step with the same force
        s.step(same, AC.NSTEPS)
        s.ghat = None
        assert torch.equal(same.what, state.what) and torch.equal(same.that, state.that)
        wbar, tbar, gbar = adjoint(s, what0, that0, mean, ghat, s.init_vorticity(rw).what, scalar_spectrum(s, rt))
        assert torch.equal(w0.grad, s.vorticity(state_of(s, wbar))) and torch.equal(th0.grad, field_of(s, tbar))
        gf = s.vorticity(state_of(s, gbar))
        assert torch.equal(forcing.grad, torch.sum(gf, dim=0, keepdim=True) if reduce else gf)
        assert min(float(forcing.grad.abs().max()), float(w0.grad.abs().max()), float(th0.grad.abs().max())) > 0


def test_advance_velocity_scalar_gradient_against_the_oracle(gpu_device):
    c = AC.CASES[0]
    nx, ny, B = c[:3]
    d = AC.inputs(c)
    s = solver(c, d['dt'])
    u0, v0, th0 = (dev(d[k]).requires_grad_(True) for k in ('u0', 'v0', 'theta0'))
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    ru, rv = O.band_ic(B, nx, ny, 77, c[3], c[4], 1.0)
    ru, rv = ru.astype(np.float32), rv.astype(np.float32)
    u, v, th = s.advance_velocity_scalar(u0, v0, th0, AC.NSTEPS, forcing=g)
    (u * dev(ru) + v * dev(rv) + th * dev(d['rt'])).sum().backward()
    st = s.init(u0.detach(), v0.detach(), th0.detach())
    s.ghat = s.init_vorticity(g.detach()).what
    s.step(st, AC.NSTEPS)
    s.ghat = None
    fu, fv, _ = s.fields(st)
    assert torch.equal(u.detach(), fu) and torch.equal(v.detach(), fv) and torch.equal(th.detach(), s.scalar(st))
    S = AC.scheme(c, d['dt'])
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    f64 = lambda a: a.astype(np.float64)
    wbar, tbar, gbar = S.step_vjp(w, S.init_scalar(d['theta0']), mean, S.velocity_vjp(f64(ru), f64(rv)), np.fft.rfft2(f64(d['rt'])), AC.NSTEPS)
    ub, vb = S.init_vjp(wbar)
    got = lambda t: f64(t.grad.cpu().numpy())
    errs = (AC.rel(got(u0), ub), AC.rel(got(v0), vb), AC.rel(got(th0), S.irfft2(tbar)), AC.rel(got(g), S.irfft2(gbar)))
    print('MEASURED advance_velocity_scalar %s: u0 %.2e v0 %.2e theta0 %.2e g %.2e' % ((AC.case_id(c),) + errs))
    assert max(errs) <= AC.BOUND, errs


# ---------------------------------------------------------------------------------------------------- 3. against the flow's adjoint
def test_without_buoyancy_and_scalar_cotangent_the_flow_adjoint_is_the_parents(gpu_device):
    """b = 0 and mu = 0: wbar and gbar are spec_ns_step_adjoint_'s, and nothing reaches thetabar -- with G and theta and without them.  Then the
    mirror image: lam = 0 with G = 0 and theta = 0 leaves wbar at zero (the scalar's cotangent reaches the flow only through grad theta + G)."""
    from nns import ops
    c = AC.CASES[1]
    assert c[6] == AC.PASSIVE
    s, d, start, ghat, lam, mu, _, _, _ = direct(c)
    what0, that0 = forward(s, start.clone(), ghat, AC.NSTEPS)
    wbar, tbar, gbar = adjoint(s, what0, that0, start.mean, ghat, lam, torch.zeros_like(mu))
    pl, pg = lam.clone(), torch.empty_like(lam)
    work = torch.empty(ops.spec_ns_adjoint_workspace(c[2], s.nx, s.ny), dtype=torch.uint8, device='cuda')
    ops.spec_ns_step_adjoint_(what0, start.mean, ghat, pl, pg, work, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag)
    ew, eg = AC.rel(cplx(wbar), cplx(pl)), AC.rel(cplx(gbar), cplx(pg))
    print('against the flow adjoint: wbar %.2e gbar %.2e, bitwise %s' % (ew, eg, torch.equal(wbar, pl) and torch.equal(gbar, pg)))
    assert ew <= AC.BOUND and eg <= AC.BOUND
    assert torch.equal(wbar, pl) and torch.equal(gbar, pg)                   # one text of the recurrences serves both calls
    assert float(tbar.abs().max()) == 0.0 and float(that0.abs().max()) > 0
    s0 = solver(c, d['dt'], grad=(0.0, 0.0))
    rest = start.clone()
    rest.that.zero_()
    what0, that0 = forward(s0, rest, ghat, AC.NSTEPS)
    assert float(that0.abs().max()) == 0.0                                   # no gradient, no scalar: it stays away
    wbar, tbar, _ = adjoint(s0, what0, that0, start.mean, ghat, lam, torch.zeros_like(mu))
    assert float(tbar.abs().max()) == 0.0 and torch.equal(wbar, adjoint(s, what0, that0, start.mean, ghat, lam, torch.zeros_like(mu))[0])
    wbar, tbar, gbar = adjoint(s0, what0, that0, start.mean, ghat, torch.zeros_like(lam), mu)
    assert float(wbar.abs().max()) == 0.0 and float(gbar.abs().max()) == 0.0 and float(tbar.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 4. analytic
def test_scalar_gradient_at_rest_is_the_decayed_cotangent_per_mode(gpu_device):
    """Fluid at rest, G = 0, b = 0: thetabar = exp(-kappa |k|^2 n dt) mu on every kept mode, the (0, 0) mode included.  Per step a mode is
    scaled once, mu + expm1(-kappa dt |k|^2) mu.  The argument (up to 0.67 at the band's corner here) carries the roundings of -kappa dt / 2,
    of |k|^2 and of their product, 2.5 ulp of it or 1.7 ulp of the result; expm1 gives 2 ulp of a term below the result; the multiply-add
    half an ulp: 4 ulp per step, 12 ulp = 7e-7 after three; 1e-6."""
    c = (64, 128, 2, 3.0, 7.0, (0.0, 0.0), AC.PASSIVE)
    n, dt, kappa = 3, 0.01, 2e-2
    s = solver(c, dt, nu=1e-2, drag=0.3, kappa=kappa, grad=(0.0, 0.0))
    rng = np.random.default_rng(3)
    zero = torch.zeros((2, 64, 128), device='cuda')
    state = s.init(zero, zero, dev(rng.standard_normal((2, 64, 128))))
    mu = scalar_spectrum(s, dev(rng.standard_normal((2, 64, 128))))          # white: every kept mode and a mean
    what0, that0 = forward(s, state, None, n)
    _, tbar, _ = adjoint(s, what0, that0, state.mean, None, torch.zeros_like(mu), mu, want_g=False)
    S = AC.A.ScalarAdjointScheme(64, 128, dt, 1.0, 1e-2, 3.0, 7.0, drag=0.3, kappa=kappa)
    decay = S.compact(np.exp(-kappa * S.k2 * n * dt) * S.Mt)
    ref, got = decay * cplx(mu), cplx(tbar)
    keep = S.compact(S.Mt) > 0
    err = np.abs(got - ref)[:, keep] / np.abs(ref)[:, keep]
    print('at rest: worst mode rel %.2e' % err.max())
    assert err.max() <= 1e-6 and np.all(got[:, ~keep] == 0) and abs(got[0, 0, 0]) > 0


# ---------------------------------------------------------------------------------------------------- 5. bit identities
@pytest.mark.parametrize('case', [AC.CASES[0], AC.CASES[4]], ids=AC.case_id)
def test_a_batch_is_its_grids_and_one_call_is_chained_calls(gpu_device, case):
    s, d, start, ghat, lam, mu, wbar, tbar, gbar = direct(case)
    B = case[2]
    for b in range(B):
        w1, t1, g1 = direct(case, grids=slice(b, b + 1))[6:]
        assert torch.equal(w1[0], wbar[b]) and torch.equal(t1[0], tbar[b]) and torch.equal(g1[0], gbar[b])
    what0, that0 = forward(s, start.clone(), ghat, AC.NSTEPS)
    l, m, gsum = lam, mu, None
    for k in reversed(range(AC.NSTEPS)):
        l, m, g = adjoint(s, what0[k:k + 1], that0[k:k + 1], start.mean, ghat, l, m)
        gsum = g if gsum is None else gsum + g
    assert torch.equal(l, wbar) and torch.equal(m, tbar)
    assert float((gsum - gbar).abs().max()) <= 1e-6 * float(gbar.abs().max())     # the call sums in another order: stage by stage
    lw, lt, none = adjoint(s, what0, that0, start.mean, ghat, lam, mu, want_g=False)
    assert none is None and torch.equal(lw, wbar) and torch.equal(lt, tbar)
    zw, zt, zg = adjoint(s, what0, that0, start.mean, ghat, torch.zeros_like(lam), torch.zeros_like(mu))
    assert max(float(t.abs().max()) for t in (zw, zt, zg)) == 0.0


def test_grid_stride(gpu_device):
    c = AC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = AC.C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    rw, rt = O.band_ic(4, nx, ny, 5, c[3], c[4], 1.0)
    th = O.band_ic(4, nx, ny, 6, c[3], c[4], 1.0)[0] + 0.25
    s = solver(c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]), dev(th[sel]))
        lam, mu = s.init_vorticity(dev(rw[sel])).what, scalar_spectrum(s, dev(rt[sel] + 0.1))
        what0, that0 = forward(s, state, None, 1)
        outs.append(adjoint(s, what0, that0, state.mean, None, lam, mu))
    whole, first, last = outs
    for a, f, l in zip(whole, first, last):
        assert torch.equal(a[:2], f) and torch.equal(a[-2:], l) and float(a.abs().max()) > 0


def test_the_call_stays_inside_its_workspace(gpu_device):
    """64 x 64 (the smallest grid on both axes: 22 kept columns in one 64-line tile), one grid of the buoyant case, 2 steps, gbar wanted: the
    bytes after the queried size keep their fill, and the results are those of a plain workspace of that size."""
    from nns import ops
    c = AC.CASES[0]
    assert c[6] == AC.UNSTABLE
    s, d, start, ghat, lam, mu, wbar, tbar, gbar = direct(c, nsteps=2, grids=slice(0, 1))
    what0, that0 = forward(s, start.clone(), ghat, 2)
    need = ops.spec_ns_scalar_adjoint_workspace(1, s.nx, s.ny)
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    w2, t2, g2 = adjoint(s, what0, that0, start.mean, ghat, lam, mu, work=buf[:need])
    assert bool((buf[need:] == 0xA5).all())
    assert torch.equal(w2, wbar) and torch.equal(t2, tbar) and torch.equal(g2, gbar) and float(gbar.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_solvers_outside_the_adjoint_are_refused(gpu_device):
    c = (64, 64, 1, TWO_PI, TWO_PI, (0.0, 0.0), AC.UNSTABLE)
    w = torch.zeros((1, 64, 64), device='cuda', requires_grad=True)
    from nns.periodic import PeriodicSolver
    bare = PeriodicSolver(64, 64, 0.01, 1.0, 1e-3)
    for call in (lambda s: s.advance_scalar(w, w, 1), lambda s: s.advance_velocity_scalar(w, w, w, 1)):
        with pytest.raises(ValueError, match='kappa'):
            call(bare)
        for kw, name in ((dict(hyperviscosity=(1e-8, 2)), 'hyperviscosity'), (dict(hypofriction=(0.1, 1)), 'hypofriction'), (dict(beta=1.0), 'beta'),
                         (dict(), 'set_stochastic_forcing')):
            s = solver(c, 0.01, **kw)
            if name == 'set_stochastic_forcing':
                s.ring_forcing(1.0, 3.0, 5.0)
            with pytest.raises(NotImplementedError, match=name):
                call(s)
    s = solver(c, 0.01)
    ok = torch.zeros((1, 64, 64), device='cuda')
    with pytest.raises(TypeError):
        s.advance_scalar(ok, torch.zeros(1, 64, 64), 1)
    with pytest.raises(TypeError):
        s.advance_scalar(ok.double(), ok, 1)
    with pytest.raises(TypeError):
        s.advance_scalar(ok, ok, 1, forcing=torch.zeros(1, 64, 64))
    with pytest.raises(ValueError):
        s.advance_scalar(ok, torch.zeros((2, 64, 64), device='cuda'), 1)
    with pytest.raises(ValueError):
        s.advance_scalar(ok, ok, 1, forcing=torch.zeros((3, 64, 64), device='cuda'))
    with pytest.raises(ValueError):
        s.advance_scalar(ok, ok, 0)
    with pytest.raises(ValueError):
        s.advance_velocity_scalar(ok, ok, torch.zeros((1, 64, 128), device='cuda'), 1)


def test_c_entry_points_refuse_before_any_launch(gpu_device):
    """NULL, a short workspace, a non-finite kappa, G or b: the buffers are poisoned and must come back untouched."""
    from nns import _lib, ops
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_spec_ns_scalar_adjoint_workspace(2, 64, 64, ctypes.byref(n)) == 0
    assert n.value == max(21 * 2 * 64 * 22 * 8, ops.spec_ns_workspace(2, 64, 64))          # 21 compacted fields, and it serves the other calls
    assert n.value >= ops.spec_ns_adjoint_workspace(2, 64, 64) and n.value >= ops.spec_ns_scalar_workspace(2, 64, 64)
    assert L.nns_spec_ns_scalar_adjoint_workspace(2, 64, 64, None) == INVALID
    assert L.nns_spec_ns_scalar_adjoint_workspace(2, 96, 64, ctypes.byref(n)) != 0
    t = torch.full((n.value,), 7, dtype=torch.uint8, device='cuda')
    P = t.data_ptr()

    def args(what0=P, that0=P, lam=P, mu=P, work=P, nbytes=n.value, kappa=1e-3, gx=0.1, by=0.5):
        return (what0, that0, P, None, 0, lam, mu, None, work, nbytes, 2, 64, 64, TWO_PI, TWO_PI, 0.01, 1e-3, 0.0, kappa, gx, 0.0, 0.0, by, 1, None)

    call = L.nns_spec_ns_step_scalar_adjoint_f32
    for bad in (dict(what0=None), dict(that0=None), dict(lam=None), dict(mu=None), dict(work=None)):
        assert call(*args(**bad)) == INVALID
    assert call(*args(nbytes=n.value - 1)) == WORKSPACE
    assert b'nns_spec_ns_scalar_adjoint_workspace' in L.nns_last_error()
    for bad in (dict(by=float('nan')), dict(by=float('inf')), dict(gx=float('nan')), dict(kappa=float('inf')), dict(kappa=-1.0)):
        assert call(*args(**bad)) == INVALID
    torch.cuda.synchronize()
    assert bool((t == 7).all())
