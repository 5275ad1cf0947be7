"""GPU checks of the reverse mode of the periodic solver's linear step and of the complete entry points (csrc/pspec_kernels.hip:
nns_spec_ns_step_linear_adjoint_f32, ps_col_adj_kernel with a PsAdjLinear / PsAdjScalarLinear, ps_col_kernel with a PsLinear and a PsKeep;
nns.periodic.PeriodicSolver.evolve / evolve_velocity) against the float64 restatement tests/pspec_linear_adjoint_oracle.py, the existing
adjoints and its own bit identities.  Inputs fill the whole 2/3 band (tests/pspec_linear_adjoint_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_cases as C
import pspec_linear_adjoint_cases as LA
import pspec_oracle as O

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi
NSTEPS = LA.NSTEPS


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def cplx(t):
    w = t.cpu().numpy().astype(np.float64)
    return w[..., 0] + 1j * w[..., 1]


def is_scalar(kind):
    return kind in ('scalar', 'buoyant')


def scalar_spectrum(s, field):
    """M_theta rfft2 of a field [B, nx, ny] in the state's layout: the scalar's compact kernel."""
    from nns import ops
    B = field.shape[0]
    work = torch.empty(ops.spec_ns_scalar_workspace(B, s.nx, s.ny), dtype=torch.uint8, device='cuda')
    return ops.spec_ns_scalar_init(field.contiguous(), torch.empty((B, s.my1, s.nx, 2), dtype=torch.float32, device='cuda'), work)


def forward(s, state, ghat, nsteps):
    """(what0, that0 or None) [nsteps, B, my1, nx, 2] of nsteps steps of the state (advanced in place) by the solver's own ``step`` under the
    force spectrum ghat."""
    what0 = torch.empty((nsteps,) + tuple(state.what.shape), dtype=torch.float32, device='cuda')
    that0 = None if state.that is None else torch.empty_like(what0)
    keep, s.ghat = s.ghat, ghat
    try:
        for k in range(nsteps):
            what0[k].copy_(state.what)
            if that0 is not None:
                that0[k].copy_(state.that)
            s.step(state, 1)
    finally:
        s.ghat = keep
    return what0, that0


def table(s):
    """The solver's table (Re, Im)(lambda dt / 2) on the device; on a solver without the three terms it holds nu and the drag alone."""
    return torch.from_numpy(s._linear_table()).cuda()


def adjoint(s, what0, that0, mean, ghat, lam, mu, want_g=True, work=None, linear=None):
    """(wbar, thetabar or None, gbar) of the direct adjoint call: the linear one on a solver with the general linear operator (or with
    linear = True), else the existing ones.  lam and mu are not modified.  work: the workspace (None: a fresh one of the queried size)."""
    from nns import ops
    B = lam.shape[0]
    lam, mu = lam.clone(), None if mu is None else mu.clone()
    gbar = torch.full_like(lam, float('nan')) if want_g else None            # overwritten, not added to
    if work is None:
        size = ops.spec_ns_adjoint_workspace if that0 is None else ops.spec_ns_scalar_adjoint_workspace
        work = torch.empty(size(B, s.nx, s.ny), dtype=torch.uint8, device='cuda')
    box = (s.ny, s.Lx, s.Ly, s.dt)
    if s._linear() if linear is None else linear:
        ops.spec_ns_step_linear_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, *box, 0.0 if s.kappa is None else s.kappa,
                                         s.scalar_gradient, s.buoyancy, table(s))
    elif that0 is None:
        ops.spec_ns_step_adjoint_(what0, mean, ghat, lam, gbar, work, *box, s.nu, s.drag)
    else:
        ops.spec_ns_step_scalar_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, *box, s.nu, s.drag, s.kappa, s.scalar_gradient, s.buoyancy)
    return lam, mu, gbar


def start_state(s, kind, d, pick=lambda a: a, clock=0, ids=None):
    """The state of a run's inputs; a stochastic one with the given clock and grid ids."""
    th = dev(pick(d['theta0'])) if is_scalar(kind) else None
    state = s.init(dev(pick(d['u0'])), dev(pick(d['v0'])), th)
    if kind == 'stochastic':
        state.clock = torch.full((1,), clock, dtype=torch.int64, device='cuda')
        if ids is not None:
            state.noise_ids = torch.as_tensor(ids, dtype=torch.int32, device='cuda')
    return state


def direct(kind, c, nsteps=NSTEPS, grids=None, linear=True):
    """(s, d, start, ghat, lam, mu, wbar, thetabar, gbar) of the run through the C-level call; grids: a slice of the batch run alone (with its
    own noise ids)."""
    d = LA.inputs(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = LA.solver(kind, c, d['dt'], linear)
    ghat = s.init(dev(pick(d['fx'])), dev(pick(d['fy']))).what
    state = start_state(s, kind, d, pick, ids=None if grids is None else np.arange(c[2])[grids])
    start = state.clone()
    lam = s.init_vorticity(dev(pick(d['rw']))).what
    mu = scalar_spectrum(s, dev(pick(d['rt']))) if is_scalar(kind) else None
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
    from nns import ops
    return ops.spec_ns_scalar_field(that, state_of(s, that).work, s.ny)


# ---------------------------------------------------------------------------------------------------- 1. against the float64 restatement
@pytest.mark.parametrize('run', LA.RUNS, ids=LA.run_id)
def test_gradient_against_the_oracle(gpu_device, run):
    kind, case = run
    s, d, start, ghat, lam, mu, wbar, tbar, gbar = direct(kind, case)
    assert s._linear() and (s.stoch_amp is not None) == (kind == 'stochastic')
    got = (wbar, tbar, gbar) if is_scalar(kind) else (wbar, gbar)
    errs = tuple(LA.rel(cplx(g), r) for g, r in zip(got, LA.oracle_gradient(kind, case)))
    print('MEASURED %s: %s' % (LA.run_id(run), ' '.join('%.2e' % e for e in errs)))
    assert max(errs) <= LA.bound(kind), errs


def test_evolve_velocity_gradient_against_the_oracle(gpu_device):
    """The buoyant linear run from and to the velocity: forward bitwise fields(step(init)), gradients of (u0, v0, theta0, forcing)."""
    kind, c = 'buoyant', LA.CASES[0]
    nx, ny, B = c[:3]
    d = LA.inputs(c)
    s = LA.solver(kind, c, d['dt'])
    u0, v0, th0 = (dev(d[k]).requires_grad_(True) for k in ('u0', 'v0', 'theta0'))
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    ru, rv = O.band_ic(B, nx, ny, 77, c[3], c[4], 1.0)
    ru, rv = ru.astype(np.float32), rv.astype(np.float32)
    u, v, th = s.evolve_velocity(u0, v0, NSTEPS, theta0=th0, forcing=g)
    (u * dev(ru) + v * dev(rv) + th * dev(d['rt'])).sum().backward()
    st = s.init(u0.detach(), v0.detach(), th0.detach())
    s.ghat = s.init_vorticity(g.detach()).what
    s.step(st, NSTEPS)
    s.ghat = None
    fu, fv, _ = s.fields(st)
    assert torch.equal(u.detach(), fu) and torch.equal(v.detach(), fv) and torch.equal(th.detach(), s.scalar(st))
    S = LA.scheme(kind, c, d['dt'])
    S.set_forcing(d['fx'], d['fy'])
    w, mean = S.init(d['u0'], d['v0'])
    f64 = lambda a: a.astype(np.float64)
    wbar, tbar, gbar = S.step_vjp(w, mean, S.velocity_vjp(f64(ru), f64(rv)), NSTEPS, t=S.init_scalar(d['theta0']), mu=np.fft.rfft2(f64(d['rt'])))
    ub, vb = S.init_vjp(wbar)
    got = lambda t: f64(t.grad.cpu().numpy())
    errs = (LA.rel(got(u0), ub), LA.rel(got(v0), vb), LA.rel(got(th0), S.irfft2(tbar)), LA.rel(got(g), S.irfft2(gbar)))
    print('MEASURED evolve_velocity %s: u0 %.2e v0 %.2e theta0 %.2e g %.2e' % ((LA.run_id((kind, c)),) + errs))
    assert max(errs) <= LA.BOUND_SCALAR, errs


# ---------------------------------------------------------------------------------------------------- 2. the autograd path
PERM = (2, 0, 1)


@pytest.mark.parametrize('kind,linear', [('flow', True), ('buoyant', True), ('stochastic', True), ('stochastic', False)],
                         ids=['flow', 'buoyant', 'stochastic', 'stochastic-forced'])
def test_evolve_is_step_and_its_backward_the_direct_adjoint_call_bitwise(gpu_device, kind, linear):
    """Forward: the bits of ``step`` on the same state (one call of NSTEPS steps; the stochastic run with clock = 5 and permuted ids).  Backward:
    the bits of the direct call on the start spectra the forward saved -- the linear adjoint, or for the stochastic step without a table the
    existing forced adjoint: the generator is not part of it.  Shared and per-grid ``forcing``."""
    c = LA.CASES[0]
    d = LA.inputs(c)
    s = LA.solver(kind, c, d['dt'], linear)
    assert s._linear() == linear
    sc = is_scalar(kind)
    noise = dict(clock=5, noise_ids=PERM) if kind == 'stochastic' else {}
    st = start_state(s, kind, d)
    w0 = s.vorticity(st).requires_grad_(True)
    th0 = dev(d['theta0']).requires_grad_(True) if sc else None
    mean = st.mean.clone()
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy'])))
    rw, rt = dev(d['rw']), dev(d['rt'])
    for forcing, reduce in ((g.clone().requires_grad_(True), False), (g[:1].clone().requires_grad_(True), True)):
        w0.grad = None
        if sc:
            th0.grad = None
            ow, ot = s.evolve(w0, NSTEPS, theta=th0, mean=mean, forcing=forcing)
            ((ow * rw).sum() + (ot * rt).sum()).backward()
        else:
            ow = s.evolve(w0, NSTEPS, mean=mean, forcing=forcing, **noise)
            (ow * rw).sum().backward()
        state = s.init_vorticity(w0.detach(), mean)
        if sc:
            state.that = scalar_spectrum(s, th0.detach())
        if kind == 'stochastic':
            state.clock = torch.full((1,), 5, dtype=torch.int64, device='cuda')
            state.noise_ids = torch.as_tensor(PERM, dtype=torch.int32, device='cuda')
        same = state.clone()
        ghat = s.init_vorticity(forcing.detach()).what
        what0, that0 = forward(s, state, ghat, NSTEPS)
        assert torch.equal(ow.detach(), s.vorticity(state)) and (not sc or torch.equal(ot.detach(), s.scalar(state)))
        s.ghat = ghat                                                 # one call of NSTEPS steps
        s.step(same, NSTEPS)
        s.ghat = None
        assert torch.equal(same.what, state.what) and (not sc or torch.equal(same.that, state.that))
        if kind == 'stochastic':
            assert int(same.clock.item()) == 5 + NSTEPS
            plain = s.init_vorticity(w0.detach(), mean)               # clock 0, ids arange: other noise
            s.ghat = ghat
            s.step(plain, NSTEPS)
            s.ghat = None
            assert not torch.equal(plain.what, state.what)
        wbar, tbar, gbar = adjoint(s, what0, that0, mean, ghat, s.init_vorticity(rw).what, scalar_spectrum(s, rt) if sc else None)
        assert torch.equal(w0.grad, s.vorticity(state_of(s, wbar))) and (not sc or torch.equal(th0.grad, field_of(s, tbar)))
        gf = s.vorticity(state_of(s, gbar))
        assert torch.equal(forcing.grad, torch.sum(gf, dim=0, keepdim=True) if reduce else gf)
        assert min(float(forcing.grad.abs().max()), float(w0.grad.abs().max())) > 0 and bool(torch.isfinite(w0.grad).all())


def test_the_clock_may_be_a_device_tensor_that_is_not_advanced(gpu_device):
    c = LA.CASES[0]
    d = LA.inputs(c)
    s = LA.solver('stochastic', c, d['dt'])
    w0 = s.vorticity(s.init(dev(d['u0']), dev(d['v0'])))
    clock = torch.full((1,), 5, dtype=torch.int64, device='cuda')
    a = s.evolve(w0, 2, clock=clock, noise_ids=torch.as_tensor(PERM))
    assert int(clock.item()) == 5 and torch.equal(a, s.evolve(w0, 2, clock=5, noise_ids=list(PERM)))
    assert not torch.equal(a, s.evolve(w0, 2, clock=5))
    with pytest.raises(ValueError):
        s.evolve(w0, 1, clock=-1)
    with pytest.raises(ValueError):
        s.evolve(w0, 1, noise_ids=[0, 1])
    with pytest.raises(TypeError):
        s.evolve(w0, 1, clock=0.5)
    quiet = LA.solver('flow', c, d['dt'])                              # no stochastic force: both are ignored
    assert torch.equal(quiet.evolve(w0, 1, clock=9, noise_ids=[7]), quiet.evolve(w0, 1))


# ---------------------------------------------------------------------------------------------------- 3. against the old entry points
def grads_of(out, weights, leaves):
    for t in leaves:
        t.grad = None
    sum((o * r).sum() for o, r in zip(out, weights)).backward()
    return [t.grad.clone() for t in leaves]


@pytest.mark.parametrize('kind', ['flow', 'buoyant'])
def test_on_a_solver_the_old_entry_points_accept_evolve_is_theirs_bitwise(gpu_device, kind):
    """Outputs and every gradient (w or u0, v0; theta; forcing), from the vorticity and from the velocity."""
    c = LA.CASES[0]
    d = LA.inputs(c)
    s = LA.solver(kind, c, d['dt'], linear=False)
    sc = is_scalar(kind)
    st = s.init(dev(d['u0']), dev(d['v0']))
    mean = st.mean.clone()
    w0 = s.vorticity(st).requires_grad_(True)
    u0, v0, th0 = (dev(d[k]).requires_grad_(True) for k in ('u0', 'v0', 'theta0'))
    f = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    rw, rt, ru = dev(d['rw']), dev(d['rt']), dev(d['fx'])
    if sc:
        old = s.advance_scalar(w0, th0, NSTEPS, mean=mean, forcing=f)
        go = grads_of(old, (rw, rt), (w0, th0, f))
        new = s.evolve(w0, NSTEPS, theta=th0, mean=mean, forcing=f)
        gn = grads_of(new, (rw, rt), (w0, th0, f))
        oldv = s.advance_velocity_scalar(u0, v0, th0, NSTEPS, forcing=f)
        gov = grads_of(oldv, (ru, rw, rt), (u0, v0, th0, f))
        newv = s.evolve_velocity(u0, v0, NSTEPS, theta0=th0, forcing=f)
        gnv = grads_of(newv, (ru, rw, rt), (u0, v0, th0, f))
    else:
        old = (s.advance(w0, NSTEPS, mean=mean, forcing=f),)
        go = grads_of(old, (rw,), (w0, f))
        new = (s.evolve(w0, NSTEPS, mean=mean, forcing=f),)
        gn = grads_of(new, (rw,), (w0, f))
        oldv = s.advance_velocity(u0, v0, NSTEPS, forcing=f)
        gov = grads_of(oldv, (ru, rw), (u0, v0, f))
        newv = s.evolve_velocity(u0, v0, NSTEPS, forcing=f)
        gnv = grads_of(newv, (ru, rw), (u0, v0, f))
    for a, b in zip(tuple(old) + tuple(oldv) + tuple(go) + tuple(gov), tuple(new) + tuple(newv) + tuple(gn) + tuple(gnv)):
        assert torch.equal(a, b) and float(a.detach().abs().max()) > 0
    with pytest.raises(ValueError, match='theta'):                    # theta is required iff the solver has kappa
        s.evolve(w0, 1) if sc else s.evolve(w0, 1, theta=w0)


@pytest.mark.parametrize('kind', ['flow', 'buoyant'])
def test_a_table_of_viscosity_and_drag_alone_agrees_with_the_existing_adjoint(gpu_device, kind):
    """nu_h = mu = beta = 0: the table holds lambda dt / 2 = -(nu |k|^2 + drag) dt / 2, and the linear adjoint is the existing one evaluated
    with other roundings of the same factors.  Bound: the table entry is the float32 rounding of the float64 value (half an ulp), the real
    kernels' own x = hnudt |k|^2 - hdrag carries 2.5 ulp (the roundings of hnudt, of |k|^2 and of their product); expm1f gives 2 ulp of E - 1,
    and E^2 - 1 comes as (E - 1)(E + 1) (3 more ulp of it, |E^2 - 1| <= 2 |x|) where the real form takes expm1(2 x) (2 ulp): relative to a
    factor that is (3 + 2 + 2 (3 + 2)) = 15 ulp |x|, rounded to 16; a cotangent passes E^2 once in the recomputed stages and once in the
    adjoint per step, 4 factors E, so 16 ulp x 4 x NSTEPS x max |x| bounds the relative change of any mode, hence the rel-L2 of the whole
    (ulp = 2^-23)."""
    c = LA.CASES[0]
    s, d, start, ghat, lam, mu, wbar, tbar, gbar = direct(kind, c, linear=False)
    assert not s._linear()
    what0, that0 = forward(s, start.clone(), ghat, NSTEPS)
    lw, lt, lg = adjoint(s, what0, that0, start.mean, ghat, lam, mu, linear=True)
    xmax = float(np.abs(s._linear_table()[..., 0]).max())
    assert float(np.abs(s._linear_table()[..., 1]).max()) == 0.0 and xmax > 0
    bound = 16 * 2.0 ** -23 * 4 * NSTEPS * xmax
    pairs = [(lw, wbar), (lg, gbar)] + ([(lt, tbar)] if is_scalar(kind) else [])
    errs = [LA.rel(cplx(a), cplx(b)) for a, b in pairs]
    print('table of nu and drag alone (%s): max |x| %.3f, bound %.2e, rel %s' % (kind, xmax, bound, ' '.join('%.2e' % e for e in errs)))
    assert max(errs) <= bound, (errs, bound)


# ---------------------------------------------------------------------------------------------------- 4. stochastic rollouts
@pytest.mark.parametrize('linear', [True, False], ids=['linear', 'forced'])
def test_a_stochastic_rollout_in_chunks_reproduces_the_uncut_noise(gpu_device, linear):
    """Two chunks of 2 steps with clock = 0, 2 against one call of 4 steps, gradients chained through.  Between the chunks the state is handed
    over as a FIELD (irfft2, then rfft2 of it in the next call), which is not a bit-exact round trip of the spectrum: the chunked rollout is
    bitwise the state-level run that makes the same hand-over and continues the clock -- every kick is the uncut run's, bit for bit -- and
    equals the uncut call to the project's bound for a float32 trajectory (pspec_cases.BOUND_W) and its gradient to twice the adjoint's bound
    (both are float32 evaluations within that bound of one float64 gradient).  With the second chunk's clock left at 0 the noise repeats and
    the result is far away."""
    c = LA.CASES[0]
    d = LA.inputs(c)
    s = LA.solver('stochastic', c, d['dt'], linear)
    st = s.init(dev(d['u0']), dev(d['v0']))
    mean, rw = st.mean.clone(), dev(d['rw'])
    w0 = s.vorticity(st).requires_grad_(True)
    whole = s.evolve(w0, 4, mean=mean, noise_ids=PERM)
    (g_whole,) = torch.autograd.grad((whole * rw).sum(), w0)
    half = s.evolve(w0, 2, mean=mean, clock=0, noise_ids=PERM)
    cut = s.evolve(half, 2, mean=mean, clock=2, noise_ids=PERM)
    (g_cut,) = torch.autograd.grad((cut * rw).sum(), w0)
    state = s.init_vorticity(w0.detach(), mean)
    state.clock = torch.zeros(1, dtype=torch.int64, device='cuda')
    state.noise_ids = torch.as_tensor(PERM, dtype=torch.int32, device='cuda')
    s.step(state, 2)
    again = s.init_vorticity(s.vorticity(state), mean)                # the hand-over as a field
    again.clock, again.noise_ids = state.clock, state.noise_ids       # the clock goes on: 2
    assert int(again.clock.item()) == 2
    s.step(again, 2)
    assert torch.equal(cut.detach(), s.vorticity(again))
    rel = lambda a, b: float((a - b).norm() / b.norm())
    ew, eg = rel(cut.detach(), whole.detach()), rel(g_cut, g_whole)
    repeated = s.evolve(half, 2, mean=mean, clock=0, noise_ids=PERM)
    er = rel(repeated.detach(), whole.detach())
    print('chunks against the uncut call (%s): w %.2e (bitwise %s), gradient %.2e; with a repeated clock %.2e'
          % ('linear' if linear else 'forced', ew, torch.equal(cut, whole), eg, er))
    assert ew <= C.BOUND_W and eg <= 2 * LA.BOUND_FLOW
    assert er > 1e3 * C.BOUND_W


# ---------------------------------------------------------------------------------------------------- 5. bit identities
@pytest.mark.parametrize('kind', ['flow', 'buoyant', 'stochastic'])
def test_a_batch_is_its_grids_and_one_call_is_chained_calls(gpu_device, kind):
    c = LA.CASES[0]
    s, d, start, ghat, lam, mu, wbar, tbar, gbar = direct(kind, c)
    sc = is_scalar(kind)
    for b in range(c[2]):
        w1, t1, g1 = direct(kind, c, grids=slice(b, b + 1))[6:]
        assert torch.equal(w1[0], wbar[b]) and torch.equal(g1[0], gbar[b]) and (not sc or torch.equal(t1[0], tbar[b]))
    what0, that0 = forward(s, start.clone(), ghat, NSTEPS)
    l, m, gsum = lam, mu, None
    for k in reversed(range(NSTEPS)):
        l, m, g = adjoint(s, what0[k:k + 1], None if that0 is None else that0[k:k + 1], start.mean, ghat, l, m)
        gsum = g if gsum is None else gsum + g
    assert torch.equal(l, wbar) and (not sc or torch.equal(m, tbar))
    assert float((gsum - gbar).abs().max()) <= 1e-6 * float(gbar.abs().max())     # the call sums in another order: stage by stage
    lw, lt, none = adjoint(s, what0, that0, start.mean, ghat, lam, mu, want_g=False)
    assert none is None and torch.equal(lw, wbar) and (not sc or torch.equal(lt, tbar))


def test_grid_stride(gpu_device):
    """More column tiles than the launch has workgroups, against the same grids run in pieces: bitwise, no oracle."""
    c = LA.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    rw = O.band_ic(4, nx, ny, 5, c[3], c[4], 1.0)[0]
    s = LA.solver('flow', c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]))
        lam = s.init_vorticity(dev(rw[sel])).what
        what0, that0 = forward(s, state, None, 1)
        wbar, _, gbar = adjoint(s, what0, that0, state.mean, None, lam, None)
        outs.append((wbar, gbar))
    whole, first, last = outs
    for a, f, l in zip(whole, first, last):
        assert torch.equal(a[:2], f) and torch.equal(a[-2:], l) and float(a.abs().max()) > 0


def test_the_call_stays_inside_its_workspace(gpu_device):
    from nns import ops
    for kind, size in (('flow', ops.spec_ns_adjoint_workspace), ('buoyant', ops.spec_ns_scalar_adjoint_workspace)):
        s, d, start, ghat, lam, mu, wbar, tbar, gbar = direct(kind, LA.CASES[0], nsteps=2, grids=slice(0, 1))
        what0, that0 = forward(s, start.clone(), ghat, 2)
        need = size(1, s.nx, s.ny)
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
        w2, t2, g2 = adjoint(s, what0, that0, start.mean, ghat, lam, mu, work=buf[:need])
        assert bool((buf[need:] == 0xA5).all())
        assert torch.equal(w2, wbar) and torch.equal(g2, gbar) and float(gbar.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_c_entry_point_refuses_before_any_launch(gpu_device):
    """NULL lin, that0 without mu (and mu without that0), a short workspace of either kind, bad axes: the buffers are poisoned and must come
    back untouched."""
    from nns import _lib, ops
    L = _lib.lib()
    flow, scal = ops.spec_ns_adjoint_workspace(2, 64, 64), ops.spec_ns_scalar_adjoint_workspace(2, 64, 64)
    t = torch.full((scal,), 7, dtype=torch.uint8, device='cuda')
    P = t.data_ptr()

    def args(what0=P, that0=P, lam=P, mu=P, work=P, nbytes=scal, lin=P, nx=64, kappa=1e-3, by=0.5, dt=0.01):
        return (what0, that0, P, None, 0, lam, mu, None, work, nbytes, 2, nx, 64, TWO_PI, TWO_PI, dt, kappa, 0.1, 0.0, 0.0, by, lin, 1, None)

    call = L.nns_spec_ns_step_linear_adjoint_f32
    assert call(*args(lin=None)) == INVALID and b'lin' in L.nns_last_error()
    assert call(*args(mu=None)) == INVALID and call(*args(that0=None)) == INVALID
    for bad in (dict(what0=None), dict(lam=None), dict(work=None), dict(dt=0.0), dict(by=float('nan')), dict(kappa=-1.0)):
        assert call(*args(**bad)) == INVALID
    assert call(*args(nbytes=scal - 1)) == WORKSPACE and b'nns_spec_ns_scalar_adjoint_workspace' in L.nns_last_error()
    assert call(*args(that0=None, mu=None, nbytes=flow - 1)) == WORKSPACE and b'nns_spec_ns_adjoint_workspace' in L.nns_last_error()
    assert call(*args(nx=96)) == UNSUPPORTED
    assert call(*args(that0=None, mu=None, kappa=float('nan'), by=float('nan'), nbytes=flow, nx=96)) == UNSUPPORTED      # ignored without a scalar
    torch.cuda.synchronize()
    assert bool((t == 7).all())
    s = LA.solver('flow', LA.CASES[0], 0.01)
    ok = torch.zeros((1, s.my1, 64, 2), device='cuda')
    what0, mean = ok[None].clone(), torch.zeros((1, 2), device='cuda')
    work = torch.empty(ops.spec_ns_scalar_adjoint_workspace(1, 64, 64), dtype=torch.uint8, device='cuda')
    tail = (work, 64, TWO_PI, TWO_PI, 0.01, 0.0, (0.0, 0.0), (0.0, 0.0))
    with pytest.raises(ValueError, match='lin'):
        ops.spec_ns_step_linear_adjoint_(what0, None, mean, None, ok.clone(), None, None, *tail, table(s)[:, :32].contiguous())
    with pytest.raises(ValueError, match='mu'):
        ops.spec_ns_step_linear_adjoint_(what0, what0, mean, None, ok.clone(), None, None, *tail, table(s))
    with pytest.raises(TypeError):
        ops.spec_ns_step_linear_adjoint_(what0, None, mean, None, ok.clone(), None, None, *tail, table(s).double())
    with pytest.raises(ValueError):
        ops.spec_ns_step_linear_adjoint_(what0[:, :, :5].contiguous(), None, mean, None, ok.clone(), None, None, *tail, table(s))


@pytest.mark.parametrize('kw,name', [(dict(hyperviscosity=(1e-8, 2)), 'hyperviscosity'), (dict(hypofriction=(0.1, 1)), 'hypofriction'),
                                     (dict(beta=1.0), 'beta'), (dict(), 'set_stochastic_forcing')])
def test_the_old_entry_points_still_refuse_and_point_at_evolve(gpu_device, kw, name):
    from nns.periodic import PeriodicSolver
    w = torch.zeros((1, 64, 64), device='cuda', requires_grad=True)
    for kappa in (None, 1e-3):
        s = PeriodicSolver(64, 64, 0.01, 1.0, 1e-3, kappa=kappa, **kw)
        if name == 'set_stochastic_forcing':
            s.ring_forcing(1.0, 3.0, 5.0)
        calls = ((lambda: s.advance(w, 1), 'evolve'), (lambda: s.advance_velocity(w, w, 1), 'evolve_velocity')) if kappa is None else \
                ((lambda: s.advance_scalar(w, w, 1), 'evolve'), (lambda: s.advance_velocity_scalar(w, w, w, 1), 'evolve_velocity'))
        for call, instead in calls:
            with pytest.raises(NotImplementedError, match=name) as e:
                call()
            assert 'use %s,' % instead in str(e.value)
        out = s.evolve(w, 1) if kappa is None else s.evolve(w, 1, theta=w)[0]      # and the complete entry point takes the same solver
        assert bool(torch.isfinite(out).all())
