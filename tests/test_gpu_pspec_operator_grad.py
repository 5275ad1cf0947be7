"""GPU checks of the periodic solver's reverse mode in its linear operator (csrc/pspec_kernels.hip: nns_spec_ns_step_operator_adjoint_f32,
ps_col_adj_kernel with a PsAdjOperator / PsAdjScalarOperator; nns.periodic.PeriodicSolver.evolve / evolve_velocity with ``operator``,
``operator_table``, ``mode_table``) against the float64 restatement tests/pspec_operator_grad_oracle.py, the call without the table's
gradient and its own bit identities.  Inputs fill the whole 2/3 band (tests/pspec_operator_grad_cases.py)."""
import numpy as np
import pytest
import torch

import pspec_cases as C
import pspec_linear_adjoint_cases as LA
import pspec_operator_grad_cases as OC
import pspec_oracle as O
import test_gpu_pspec_linear_adjoint as T
from test_gpu_pspec_linear_adjoint import dev, cplx, is_scalar

pytestmark = pytest.mark.gpu

INVALID = -1
TWO_PI = 2 * np.pi
NSTEPS = OC.NSTEPS


def operator_adjoint(s, what0, that0, mean, ghat, lam, mu, want_g=True, want_l=True, work=None, lin=None):
    """(wbar, thetabar or None, gbar, lbar) of the direct call; lam and mu are not modified, gbar and lbar start as NaN (overwritten, not
    added to)."""
    from nns import ops
    B = lam.shape[0]
    lam, mu = lam.clone(), None if mu is None else mu.clone()
    gbar = torch.full_like(lam, float('nan')) if want_g else None
    lbar = torch.full_like(lam, float('nan')) if want_l else None
    if work is None:
        size = ops.spec_ns_adjoint_workspace if that0 is None else ops.spec_ns_scalar_adjoint_workspace
        work = torch.empty(size(B, s.nx, s.ny), dtype=torch.uint8, device='cuda')
    ops.spec_ns_step_operator_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, s.ny, s.Lx, s.Ly, s.dt, 0.0 if s.kappa is None else s.kappa,
                                       s.scalar_gradient, s.buoyancy, T.table(s) if lin is None else lin, lbar)
    return lam, mu, gbar, lbar


def direct(kind, c, nsteps=NSTEPS, grids=None):
    """dict of the run through the C-level call (s, start, ghat, lam, mu, what0, that0, wbar, tbar, gbar, lbar); grids: a slice of the batch
    run alone (with its own noise ids)."""
    d = OC.inputs(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = LA.solver(kind, c, d['dt'])
    ghat = s.init(dev(pick(d['fx'])), dev(pick(d['fy']))).what
    state = T.start_state(s, kind, d, pick, ids=None if grids is None else np.arange(c[2])[grids])
    start = state.clone()
    lam = s.init_vorticity(dev(pick(d['rw']))).what
    mu = T.scalar_spectrum(s, dev(pick(d['rt']))) if is_scalar(kind) else None
    what0, that0 = T.forward(s, state, ghat, nsteps)
    wbar, tbar, gbar, lbar = operator_adjoint(s, what0, that0, state.mean, ghat, lam, mu)
    return dict(s=s, d=d, start=start, ghat=ghat, lam=lam, mu=mu, what0=what0, that0=that0, wbar=wbar, tbar=tbar, gbar=gbar, lbar=lbar)


def kept(s):
    return torch.from_numpy(np.ascontiguousarray(s._shell_table()[3])).cuda()


def check_definition(s, G):
    """A table gradient [my1, nx, 2]: zero off the kept modes and at (0, 0), l(-k) = conj(l(k)) on the ky = 0 line to the bit."""
    assert bool(torch.isfinite(G).all()) and float(G.abs().max()) > 0
    assert bool((G[~kept(s)] == 0).all()) and bool((G[0, 0] == 0).all())
    flip = (-torch.arange(s.nx, device=G.device)) % s.nx
    assert torch.equal(G[0, :, 0], G[0, flip, 0]) and torch.equal(G[0, :, 1], -G[0, flip, 1])
    assert float(G[0].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 1. against the float64 restatement
@pytest.mark.parametrize('run', OC.RUNS, ids=OC.run_id)
def test_table_gradient_against_the_oracle(gpu_device, run):
    kind, case = run
    r = direct(kind, case)
    s, lbar = r['s'], r['lbar']
    assert bool(torch.isfinite(lbar).all()) and bool((lbar[:, ~kept(s)] == 0).all())
    G = s._operator_gradient(lbar)
    check_definition(s, G)
    err = OC.rel(cplx(G), OC.table_gradient(kind, case))
    print('MEASURED %s: %.2e' % (OC.run_id(run), err))
    assert err <= OC.bound(kind), err


def test_parameter_gradients_through_operator_table(gpu_device):
    """d L / d (nu, drag, nu_h, mu, beta) from backward() through ``operator_table`` and ``evolve``, each against the oracle's under the
    table's bound relative to its own size; the table of the solver's own numbers is the solver's table to the bit."""
    kind, c = 'flow', OC.CASES[0]
    d = OC.inputs(c)
    s = LA.solver(kind, c, d['dt'])
    assert torch.equal(s.operator_table(device='cuda').cpu(), torch.from_numpy(s._linear_table()))
    leaf = lambda x: torch.tensor(x, dtype=torch.float64, device='cuda', requires_grad=True)
    p = dict(nu=leaf(s.nu), drag=leaf(s.drag), nu_h=leaf(s.hyperviscosity[0]), mu=leaf(s.hypofriction[0]), beta=leaf(s.beta))
    table = s.operator_table(nu=p['nu'], drag=p['drag'], hyperviscosity=(p['nu_h'], s.hyperviscosity[1]),
                             hypofriction=(p['mu'], s.hypofriction[1]), beta=p['beta'], device='cuda')
    assert table.dtype == torch.float32 and torch.equal(table.detach().cpu(), torch.from_numpy(s._linear_table()))
    st = s.init(dev(d['u0']), dev(d['v0']))
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy'])))
    out = s.evolve(s.vorticity(st), NSTEPS, mean=st.mean.clone(), forcing=g, operator=table)
    (out * dev(d['rw'])).sum().backward()
    ref = OC.parameter_gradients(kind, c)
    errs = {k: abs(float(p[k].grad) - ref[k]) / abs(ref[k]) for k in OC.PARAMETERS}
    print('MEASURED parameters %s: %s' % (OC.run_id((kind, c)), ' '.join('%s %.2e (%.4g)' % (k, errs[k], ref[k]) for k in OC.PARAMETERS)))
    assert max(errs.values()) <= OC.bound(kind), errs


def test_evolve_velocity_with_operator_on_the_buoyant_run(gpu_device):
    """From and to the velocity with the scalar and the buoyancy: the table's gradient against the oracle, the outputs and the gradients of
    (u0, v0, theta0, forcing) bitwise those of the call without ``operator`` (the table is the solver's own)."""
    kind, c = 'buoyant', OC.CASES[0]
    nx, ny, B = c[:3]
    d = OC.inputs(c)
    s = LA.solver(kind, c, d['dt'])
    u0, v0, th0 = (dev(d[k]).requires_grad_(True) for k in ('u0', 'v0', 'theta0'))
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    ru, rv = O.band_ic(B, nx, ny, 77, c[3], c[4], 1.0)
    ru, rv = ru.astype(np.float32), rv.astype(np.float32)
    table = T.table(s).requires_grad_(True)
    leaves = (u0, v0, th0, g)
    weights = (dev(ru), dev(rv), dev(d['rt']))
    out = s.evolve_velocity(u0, v0, NSTEPS, theta0=th0, forcing=g, operator=table)
    grads = T.grads_of(out, weights, leaves + (table,))
    plain = s.evolve_velocity(u0, v0, NSTEPS, theta0=th0, forcing=g)
    gplain = T.grads_of(plain, weights, leaves)
    for a, b in zip(tuple(out) + tuple(grads[:4]), tuple(plain) + tuple(gplain)):
        assert torch.equal(a, b) and float(a.detach().abs().max()) > 0
    check_definition(s, grads[4])
    S, _ = OC.oracle_gradient(kind, c)
    w, mean = S.init(d['u0'], d['v0'])
    f64 = lambda a: a.astype(np.float64)
    ref = S.operator_vjp(w, mean, S.velocity_vjp(f64(ru), f64(rv)), NSTEPS, t=S.init_scalar(d['theta0']), mu=np.fft.rfft2(f64(d['rt'])))[None]
    err = OC.rel(cplx(grads[4]), S.compact(ref.sum(axis=0)))
    print('MEASURED evolve_velocity %s: %.2e' % (OC.run_id((kind, c)), err))
    assert err <= OC.BOUND_SCALAR, err


# ---------------------------------------------------------------------------------------------------- 2. the autograd path, bitwise
@pytest.mark.parametrize('kind', ['flow', 'buoyant', 'stochastic'])
def test_the_other_gradients_do_not_see_the_tables_gradient(gpu_device, kind):
    """Outputs and the gradients of the fields and of ``forcing``: operator = None, the solver's own table as a constant, and the same table
    with its gradient requested give the same bits; the table's gradient is ``_operator_gradient`` of the direct call's lbar."""
    c = OC.CASES[0]
    d = OC.inputs(c)
    s = LA.solver(kind, c, d['dt'])
    sc = is_scalar(kind)
    noise = dict(clock=5, noise_ids=T.PERM) if kind == 'stochastic' else {}
    st = T.start_state(s, kind, d)
    mean = st.mean.clone()
    w0 = s.vorticity(st).requires_grad_(True)
    th0 = dev(d['theta0']).requires_grad_(True) if sc else None
    f = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    leaves = (w0, th0, f) if sc else (w0, f)
    weights = (dev(d['rw']), dev(d['rt']))
    results = []
    for operator in (None, T.table(s), T.table(s).requires_grad_(True)):
        out = s.evolve(w0, NSTEPS, theta=th0, mean=mean, forcing=f, operator=operator, **noise)
        out = out if sc else (out,)
        want = leaves + ((operator,) if operator is not None and operator.requires_grad else ())
        results.append((out, T.grads_of(out, weights, want)))
    (o0, g0), (o1, g1), (o2, g2) = results
    for a, b, e in zip(tuple(o0) + tuple(g0), tuple(o1) + tuple(g1), tuple(o2) + tuple(g2[:len(leaves)])):
        assert torch.equal(a, b) and torch.equal(a, e) and float(a.detach().abs().max()) > 0
    state = s.init_vorticity(w0.detach(), mean)
    if sc:
        state.that = T.scalar_spectrum(s, th0.detach())
    if kind == 'stochastic':
        state.clock = torch.full((1,), 5, dtype=torch.int64, device='cuda')
        state.noise_ids = torch.as_tensor(T.PERM, dtype=torch.int32, device='cuda')
    ghat = s.init_vorticity(f.detach()).what
    what0, that0 = T.forward(s, state, ghat, NSTEPS)
    lam, mu = s.init_vorticity(weights[0]).what, T.scalar_spectrum(s, weights[1]) if sc else None
    lbar = operator_adjoint(s, what0, that0, mean, ghat, lam, mu)[3]
    assert torch.equal(g2[-1], s._operator_gradient(lbar))
    check_definition(s, g2[-1])


def test_operator_on_a_solver_without_the_linear_terms(gpu_device):
    """operator = None is the call it was (``advance``, bitwise); with a table of nu and the drag alone the call takes the linear form: the
    forced step's mathematics within the bound of test_gpu_pspec_linear_adjoint.py's table test, not its bits."""
    c = OC.CASES[0]
    d = OC.inputs(c)
    s = LA.solver('flow', c, d['dt'], linear=False)
    assert not s._linear()
    st = s.init(dev(d['u0']), dev(d['v0']))
    mean = st.mean.clone()
    w0 = s.vorticity(st).requires_grad_(True)
    rw = dev(d['rw'])
    old = s.advance(w0, NSTEPS, mean=mean)
    (go,) = T.grads_of((old,), (rw,), (w0,))
    new = s.evolve(w0, NSTEPS, mean=mean)
    (gn,) = T.grads_of((new,), (rw,), (w0,))
    assert torch.equal(old, new) and torch.equal(go, gn)
    table = s.operator_table(device='cuda').requires_grad_(True)
    assert torch.equal(table.detach().cpu(), torch.from_numpy(s._linear_table())) and float(table[..., 1].abs().max()) == 0.0
    lin = s.evolve(w0, NSTEPS, mean=mean, operator=table)
    gl, gt = T.grads_of((lin,), (rw,), (w0, table))
    xmax = float(table[..., 0].abs().max())
    bound = 16 * 2.0 ** -23 * 4 * NSTEPS * xmax
    rel = lambda a, b: float((a - b).norm() / b.norm())
    print('table of nu and drag alone: forward %.2e gradient %.2e (bound %.2e)' % (rel(lin.detach(), old.detach()), rel(gl, go), bound))
    assert rel(lin.detach(), old.detach()) <= bound and rel(gl, go) <= bound
    check_definition(s, gt)
    assert float(gt[..., 1].abs().max()) > 0                             # the flow turns modes: the loss does feel an angle


# ---------------------------------------------------------------------------------------------------- 3. bit identities of the direct call
@pytest.mark.parametrize('kind', ['flow', 'buoyant', 'stochastic'])
def test_a_batch_is_its_grids_one_call_is_chained_calls_and_a_run_repeats(gpu_device, kind):
    c = OC.CASES[0]
    r = direct(kind, c)
    s, lbar, sc = r['s'], r['lbar'], is_scalar(kind)
    for b in range(c[2]):
        one = direct(kind, c, grids=slice(b, b + 1))
        assert torch.equal(one['lbar'][0], lbar[b]) and torch.equal(one['wbar'][0], r['wbar'][b]) and torch.equal(one['gbar'][0], r['gbar'][b])
    mean = r['start'].mean
    again = operator_adjoint(s, r['what0'], r['that0'], mean, r['ghat'], r['lam'], r['mu'])
    for a, b in zip(again, (r['wbar'], r['tbar'], r['gbar'], r['lbar'])):
        assert (a is None and b is None) or torch.equal(a, b)
    l, m, lsum = r['lam'], r['mu'], None
    for k in reversed(range(NSTEPS)):
        that0 = None if r['that0'] is None else r['that0'][k:k + 1]
        l, m, g, lb = operator_adjoint(s, r['what0'][k:k + 1], that0, mean, r['ghat'], l, m)
        lsum = lb if lsum is None else lsum + lb
    assert torch.equal(l, r['wbar']) and (not sc or torch.equal(m, r['tbar']))
    assert torch.equal(lsum, lbar)
    # without lbar: the launches and the bits of the linear adjoint; with it wbar, thetabar and gbar are those too
    w0, t0, g0 = T.adjoint(s, r['what0'], r['that0'], mean, r['ghat'], r['lam'], r['mu'])
    w1, t1, g1, none = operator_adjoint(s, r['what0'], r['that0'], mean, r['ghat'], r['lam'], r['mu'], want_l=False)
    assert none is None
    for a, b, e in ((w0, w1, r['wbar']), (g0, g1, r['gbar'])) + (((t0, t1, r['tbar']),) if sc else ()):
        assert torch.equal(a, b) and torch.equal(a, e)
    only = operator_adjoint(s, r['what0'], r['that0'], mean, r['ghat'], r['lam'], r['mu'], want_g=False)
    assert only[2] is None and torch.equal(only[3], lbar) and torch.equal(only[0], r['wbar'])


def test_grid_stride(gpu_device):
    """More column tiles than the launch has workgroups, against the same grids run in pieces: bitwise, no oracle."""
    c = OC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    rw = O.band_ic(4, nx, ny, 5, c[3], c[4], 1.0)[0]
    s = LA.solver('flow', c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]))
        lam = s.init_vorticity(dev(rw[sel])).what
        what0, that0 = T.forward(s, state, None, 1)
        wbar, _, gbar, lbar = operator_adjoint(s, what0, that0, state.mean, None, lam, None)
        outs.append((wbar, lbar))
    whole, first, last = outs
    for a, f, l in zip(whole, first, last):
        assert torch.equal(a[:2], f) and torch.equal(a[-2:], l) and float(a.abs().max()) > 0


def test_the_call_stays_inside_its_workspace(gpu_device):
    """The step's own sum lives in a field of the existing workspaces: nothing is written past them."""
    from nns import ops
    for kind, size in (('flow', ops.spec_ns_adjoint_workspace), ('buoyant', ops.spec_ns_scalar_adjoint_workspace)):
        r = direct(kind, OC.CASES[0], nsteps=2, grids=slice(0, 1))
        s = r['s']
        need = size(1, s.nx, s.ny)
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
        out = operator_adjoint(s, r['what0'], r['that0'], r['start'].mean, r['ghat'], r['lam'], r['mu'], work=buf[:need])
        assert bool((buf[need:] == 0xA5).all())
        assert torch.equal(out[3], r['lbar']) and torch.equal(out[0], r['wbar']) and float(r['lbar'].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_argument_errors_raise_before_any_launch(gpu_device):
    from nns import _lib, ops
    c = OC.CASES[0]
    s = LA.solver('flow', c, 0.01)
    ok = torch.full((1, s.my1, 64, 2), 3.0, device='cuda')
    what0, mean = ok[None].clone(), torch.zeros((1, 2), device='cuda')
    work = torch.empty(ops.spec_ns_scalar_adjoint_workspace(1, 64, 64), dtype=torch.uint8, device='cuda')
    tail = (work, 64, TWO_PI, TWO_PI, 0.01, 0.0, (0.0, 0.0), (0.0, 0.0))
    lam = ok.clone()
    call = lambda lin, lbar: ops.spec_ns_step_operator_adjoint_(what0, None, mean, None, lam, None, None, *tail, lin, lbar)
    for lbar in (ok[:, :, :32].contiguous(), ok[0].clone(), ok.clone().cpu()):
        with pytest.raises((ValueError, TypeError)):
            call(T.table(s), lbar)
    with pytest.raises(TypeError):
        call(T.table(s), ok.double())
    with pytest.raises(ValueError, match='lin'):
        call(T.table(s)[:, :32].contiguous(), ok.clone())
    with pytest.raises(TypeError):
        call(T.table(s).double(), ok.clone())
    with pytest.raises(ValueError, match='mu'):
        ops.spec_ns_step_operator_adjoint_(what0, what0, mean, None, lam, None, None, *tail, T.table(s), ok.clone())
    w = torch.zeros((1, 64, 64), device='cuda', requires_grad=True)
    for bad, error in ((T.table(s)[:, :32].contiguous(), ValueError), (T.table(s).double(), TypeError), (T.table(s).cpu(), ValueError),
                       (s._linear_table(), TypeError)):
        for call_ in (lambda: s.evolve(w, 1, operator=bad), lambda: s.evolve_velocity(w, w, 1, operator=bad)):
            with pytest.raises(error, match='operator'):
                call_()
    with pytest.raises(TypeError):
        s.advance(w, 1, operator=T.table(s))                              # advance* do not take the argument
    torch.cuda.synchronize()
    assert bool((lam == 3.0).all())
    # the C entry: a NULL lin, that0 without mu; nsteps = 0 zeroes gbar and lbar and leaves lam alone
    L = _lib.lib()
    flow = ops.spec_ns_adjoint_workspace(1, 64, 64)
    P = lambda t: t.data_ptr()
    gbar, lbar, tab = torch.full_like(ok, 5.0), torch.full_like(ok, 5.0), T.table(s)

    def args(that0=None, mu=None, lin=P(tab), nsteps=1, lbar_=None):
        return (P(what0), that0, P(mean), None, 0, P(lam), mu, P(gbar), P(work), flow, 1, 64, 64, TWO_PI, TWO_PI, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0,
                lin, nsteps, None, lbar_)

    entry = L.nns_spec_ns_step_operator_adjoint_f32
    assert entry(*args(lin=None, lbar_=P(lbar))) == INVALID and b'lin' in L.nns_last_error()
    assert entry(*args(that0=P(what0), lbar_=P(lbar))) == INVALID
    torch.cuda.synchronize()
    assert bool((lam == 3.0).all()) and bool((lbar == 5.0).all()) and bool((gbar == 5.0).all())
    assert entry(*args(nsteps=0, lbar_=P(lbar))) == 0
    torch.cuda.synchronize()
    assert bool((lam == 3.0).all()) and bool((lbar == 0.0).all()) and bool((gbar == 0.0).all())


# ---------------------------------------------------------------------------------------------------- 5. what it is for
def test_mode_table_names_the_modes_of_the_table(gpu_device):
    c = OC.CASES[1]                                                      # the 1 x 4 box: anisotropic wavenumbers
    s = LA.solver('flow', c, 0.01)
    kx, ky, k2, keep = s.mode_table('cuda')
    assert all(t.shape == (s.my1, s.nx) and t.is_cuda for t in (kx, ky, k2, keep)) and keep.dtype == torch.bool
    S, shell, k2h, kepth, wt, kxh = s._shell_table()
    assert torch.equal(k2.cpu(), torch.from_numpy(k2h)) and torch.equal(keep.cpu(), torch.from_numpy(kepth))
    assert torch.equal(kx * kx + ky * ky, k2) and float(ky[1, 0]) == 2 * np.pi / c[4] and float(kx[0, 1]) == 2 * np.pi / c[3]
    # -nu |k|^2 dt / 2 written with it is the table of a solver with nu alone
    from nns.periodic import PeriodicSolver
    p = PeriodicSolver(c[0], c[1], 0.01, 1.0, 2e-3, Lx=c[3], Ly=c[4])
    mine = torch.stack([torch.where(keep, -2e-3 * k2 * (0.5 * 0.01), torch.zeros_like(k2)), torch.zeros_like(k2)], dim=-1).float()
    assert torch.allclose(mine, p.operator_table(device='cuda'), rtol=1e-6, atol=0)


def test_a_few_adam_steps_recover_viscosity_and_drag(gpu_device):
    """The inverse problem the feature is for, in small: (nu, drag) from a perturbed start against a trajectory made with the true values."""
    from nns.periodic import PeriodicSolver
    c = OC.CASES[0]
    d = OC.inputs(c)
    true = dict(nu=5e-3, drag=0.3)
    s = PeriodicSolver(c[0], c[1], d['dt'], 1.0, true['nu'], drag=true['drag'])
    st = s.init(dev(d['u0']), dev(d['v0']))
    w0, mean, nsteps = s.vorticity(st), st.mean.clone(), 6
    with torch.no_grad():
        target = s.evolve(w0, nsteps, mean=mean, operator=s.operator_table(device='cuda'))
    start = dict(nu=1.6 * true['nu'], drag=1.5 * true['drag'])      # both too damped: neither error can hide behind the other
    logs = {k: torch.tensor(np.log(v), dtype=torch.float64, device='cuda', requires_grad=True) for k, v in start.items()}
    opt = torch.optim.Adam(list(logs.values()), lr=0.05)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        table = s.operator_table(nu=logs['nu'].exp(), drag=logs['drag'].exp(), device='cuda')
        loss = ((s.evolve(w0, nsteps, mean=mean, operator=table) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    end = {k: float(v.exp()) for k, v in logs.items()}
    print('adam on (nu, drag): loss %s; nu %.3e -> %.3e (true %.3e), drag %.3f -> %.3f (true %.3f)'
          % (' '.join('%.3e' % l for l in losses), start['nu'], end['nu'], true['nu'], start['drag'], end['drag'], true['drag']))
    assert losses[-1] < losses[0]
    for k in true:
        assert abs(end[k] - true[k]) < abs(start[k] - true[k])
