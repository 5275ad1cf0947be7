"""GPU checks of the second-order adjoint of the periodic solver's step (csrc/pspec_kernels.hip: nns_spec_ns_step_second_adjoint_f32,
ps_row_adj2_kernel, the PsKeepTangent forms of ps_col_kernel, ps_col_adj_kernel with a PsAdjSecond; nns.periodic.PeriodicSolver.
second_order_forward / hessian_vector_product) against the float64 restatement tests/pspec_second_adjoint_oracle.py, the existing forward
and reverse modes (bit for bit), the symmetry of the Hessian and its own bit identities.  Inputs fill the whole 2/3 band
(tests/pspec_second_adjoint_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_oracle as O
import pspec_second_adjoint_cases as SC

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = -1, -4
TWO_PI = 2 * np.pi
FORCED, LINEAR, STOCH = (('forced', SC.CASES[0]), ('linear', SC.CASES[0]), ('stochastic', SC.CASES[0]))


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def make_solver(kind, c, dt):
    """SC.solver, and two kinds only the bit identities use: 'plain' (no drag: the unforced kernels) and 'linear-stochastic'."""
    if kind == 'plain':
        return SC.solver('forced', c, dt, drag=0.0)
    if kind == 'linear-stochastic':
        s = SC.solver('linear', c, dt)
        s.ring_forcing(*SC.LAC.ring(c), seed=SC.SEED)
        return s
    return SC.solver(kind, c, dt)


def setup(run, dg='grid', grids=None):
    """(s, kw, f): the solver of a run, the keywords of second_order_forward (mean, forcing, dforcing; no force for 'plain') and the
    case's fields on the device; grids: a slice of the batch run alone (with its own noise ids)."""
    kind, c = run
    d = SC.fields(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = make_solver(kind, c, d['dt'])
    f = {k: dev(pick(d[k])) for k in ('w', 'mean', 'g', 'dw', 'r', 'r2')}
    g = SC.dforcing(c, dg)
    kw = dict(mean=f['mean'], forcing=None if kind == 'plain' else f['g'], dforcing=dev(g if g is None or dg == 'shared' else pick(g)))
    if s.stoch_amp is not None and grids is not None:
        kw['noise_ids'] = list(range(c[2]))[grids]
    return s, kw, f


def second(run, setting, dg='grid', grids=None, nsteps=SC.NSTEPS, scale=1.0):
    """The run's SecondOrderGradients in a setting, the direction (dw, dforcing, dlam) scaled by ``scale``."""
    s, kw, f = setup(run, dg, grids)
    if kw['dforcing'] is not None:
        kw['dforcing'] = scale * kw['dforcing']
    fwd = s.second_order_forward(f['w'], scale * f['dw'], nsteps, **kw)
    dlam = scale * f['r2'] if setting == 'generic' else torch.zeros_like(f['r'])
    return fwd, fwd.backward(f['r'], dlam)


# ---------------------------------------------------------------------------------------------------- 1. against the float64 restatement
@pytest.mark.parametrize('setting', SC.SETTINGS)
@pytest.mark.parametrize('run', SC.RUNS, ids=SC.run_id)
def test_second_adjoint_against_the_oracle(gpu_device, run, setting):
    worst = [0.0, 0.0]
    for dg in (None, 'grid', 'shared'):
        out = second(run, setting, dg)[1]
        ref = SC.oracle_second(run, setting, None, dg)
        errs = SC.rel(host(out.dwbar), ref[2]), SC.rel(host(out.dgbar), ref[3])
        first = SC.rel(host(out.wbar), ref[0]), SC.rel(host(out.gbar), ref[1])
        print('MEASURED %s %s dforcing %s: dwbar %.2e dgbar %.2e (wbar %.2e gbar %.2e)' % ((SC.run_id(run), setting, dg) + errs + first))
        worst = [max(a, b) for a, b in zip(worst, errs)]
    assert max(worst) <= SC.BOUND[setting], worst


# ---------------------------------------------------------------------------------------------------- 2. the first-order outputs, bit for bit
@pytest.mark.parametrize('kind', ['plain', 'forced', 'linear', 'stochastic', 'linear-stochastic'])
def test_first_order_outputs_are_bitwise_evolve_and_evolve_tangent(gpu_device, kind):
    c = SC.CASES[0]
    s, kw, f = setup((kind, c))
    kw.update(clock=7, noise_ids=[4, 1, 9])
    w = f['w'].clone().requires_grad_(True)
    g = None if kw['forcing'] is None else kw['forcing'].clone().requires_grad_(True)
    base = {k: v for k, v in kw.items() if k != 'dforcing'}
    base['forcing'] = g
    ref = s.evolve(w, SC.NSTEPS, **base)
    (ref * f['r']).sum().backward()
    w_out, dw_out = s.evolve_tangent(f['w'], f['dw'], SC.NSTEPS, **kw)
    run = s.second_order_forward(f['w'], f['dw'], SC.NSTEPS, **kw)
    assert torch.equal(run.w, ref.detach()) and torch.equal(run.w, w_out) and torch.equal(run.dw, dw_out)
    assert tuple(run.what0.shape) == (SC.NSTEPS, c[2], s.my1, c[0], 2) == tuple(run.dwhat0.shape)
    out = run.backward(f['r'], f['r2'])
    assert torch.equal(out.wbar, w.grad) and float(out.dwbar.abs().max()) > 0
    if g is None:
        assert out.gbar is None and out.dgbar is None
    else:
        assert torch.equal(out.gbar, g.grad) and float(out.dgbar.abs().max()) > 0
    again = run.backward(f['r'], f['r2'])                                # the run is not consumed
    assert torch.equal(again.dwbar, out.dwbar) and torch.equal(again.wbar, out.wbar)


# ---------------------------------------------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize('run', [FORCED, LINEAR], ids=SC.run_id)
def test_zero_direction_gives_zero_and_doubling_doubles(gpu_device, run):
    s, kw, f = setup(run, None)
    zero = torch.zeros_like(f['dw'])
    out0 = s.second_order_forward(f['w'], zero, SC.NSTEPS, **kw).backward(f['r'], zero)
    assert float(out0.dwbar.abs().max()) == 0.0 and float(out0.dgbar.abs().max()) == 0.0
    once, twice = second(run, 'generic')[1], second(run, 'generic', scale=2.0)[1]
    assert torch.equal(out0.wbar, once.wbar) and torch.equal(out0.gbar, once.gbar)
    assert torch.equal(twice.dwbar, 2 * once.dwbar) and torch.equal(twice.dgbar, 2 * once.dgbar) and float(once.dwbar.abs().max()) > 0
    assert torch.equal(twice.wbar, once.wbar) and torch.equal(twice.gbar, once.gbar)


@pytest.mark.parametrize('kind', SC.KINDS)
def test_the_hessian_is_symmetric(gpu_device, kind):
    """<a, H b> = <b, H a> for l = 1/2 sum (w_N - obs)^2, jointly in (w, forcing): two products, float64 sums on the host."""
    c = SC.CASES[0]
    s, kw, f = setup((kind, c))
    d = SC.fields(c)
    obs = dev(O.band_ic(c[2], c[0], c[1], 77, c[3], c[4], 1.0)[0])
    loss = lambda w1: 0.5 * torch.sum((w1 - obs) ** 2)
    band = lambda a: s.vorticity(s.init_vorticity(a))                                         # band-limited, as the step takes it
    a = band(f['dw']), band(dev(d['dforcing']))
    b = band(f['r2']), band(dev(O.band_ic(c[2], c[0], c[1], 78, c[3], c[4], SC.TC.FORCE)[0]))
    base = dict(mean=kw['mean'], forcing=kw['forcing'], clock=3)
    la, ga, gfa, Ha, Hfa = s.hessian_vector_product(loss, f['w'], a[0], SC.NSTEPS, dforcing=a[1], **base)
    lb, gb, gfb, Hb, Hfb = s.hessian_vector_product(loss, f['w'], b[0], SC.NSTEPS, dforcing=b[1], **base)
    assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.equal(gfa, gfb)
    w = f['w'].clone().requires_grad_(True)
    g = kw['forcing'].clone().requires_grad_(True)
    ref = loss(s.evolve(w, SC.NSTEPS, mean=kw['mean'], forcing=g, clock=3))
    ref.backward()
    assert torch.equal(la, ref.detach()) and torch.equal(ga, w.grad) and torch.equal(gfa, g.grad)
    dot = lambda x, y: float((host(x) * host(y)).sum())
    lhs, rhs = dot(a[0], Hb) + dot(a[1], Hfb), dot(b[0], Ha) + dot(b[1], Hfa)
    scale = np.sqrt(dot(a[0], a[0]) + dot(a[1], a[1])) * np.sqrt(dot(Hb, Hb) + dot(Hfb, Hfb))
    err = abs(lhs - rhs) / scale
    print('MEASURED symmetry %s: <a, H b> %.9e <b, H a> %.9e scaled difference %.2e' % (kind, lhs, rhs, err))
    assert err <= SC.SYM_BOUND, err


def test_a_linear_loss_has_no_dlam(gpu_device):
    s, kw, f = setup(FORCED)
    l, gw, gf, hw, hf = s.hessian_vector_product(lambda w1: torch.sum(w1 * f['r']), f['w'], f['dw'], SC.NSTEPS, **kw)
    out = second(FORCED, 'pure')[1]
    assert torch.equal(hw, out.dwbar) and torch.equal(hf, out.dgbar) and torch.equal(gw, out.wbar) and torch.equal(gf, out.gbar)


@pytest.mark.parametrize('run', [FORCED, ('forced', SC.CASES[4]), STOCH], ids=SC.run_id)
def test_a_batch_is_its_grids(gpu_device, run):
    out = second(run, 'generic')[1]
    for b in range(run[1][2]):
        one = second(run, 'generic', grids=slice(b, b + 1))[1]
        for name in ('wbar', 'dwbar', 'gbar', 'dgbar'):
            assert torch.equal(getattr(one, name)[0], getattr(out, name)[b]), (b, name)


@pytest.mark.parametrize('run', [FORCED, LINEAR], ids=SC.run_id)
def test_one_call_is_chained_one_step_calls_last_first(gpu_device, run):
    from nns import ops
    s, kw, f = setup(run)
    fwd = s.second_order_forward(f['w'], f['dw'], SC.NSTEPS, **kw)
    lam0, dlam0 = s.init_vorticity(f['r']).what, s.init_vorticity(f['r2']).what
    work = torch.empty(ops.spec_ns_second_adjoint_workspace(run[1][2], s.nx, s.ny), dtype=torch.uint8, device='cuda')
    box = (work, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, fwd.lin)

    def call(what0, dwhat0, lam, dlam, gbar, dgbar):
        ops.spec_ns_second_adjoint_(what0, dwhat0, fwd.mean, fwd.ghat, fwd.dghat, lam, dlam, gbar, dgbar, *box)
    lam, dlam, gbar, dgbar = lam0.clone(), dlam0.clone(), torch.empty_like(lam0), torch.empty_like(lam0)
    call(fwd.what0, fwd.dwhat0, lam, dlam, gbar, dgbar)
    l1, d1 = lam0.clone(), dlam0.clone()
    gsum, dgsum = torch.zeros_like(lam0), torch.zeros_like(lam0)
    for k in reversed(range(SC.NSTEPS)):
        g1, dg1 = torch.empty_like(lam0), torch.empty_like(lam0)
        call(fwd.what0[k:k + 1], fwd.dwhat0[k:k + 1], l1, d1, g1, dg1)
        gsum, dgsum = gsum + g1, dgsum + dg1
    assert torch.equal(l1, lam) and torch.equal(d1, dlam) and float(dlam.abs().max()) > 0
    # the source's sums run through the steps in the one call and are added step by step here: the same terms in another order of rounding
    for part, whole in ((gsum, gbar), (dgsum, dgbar)):
        assert SC.rel(host(part), host(whole)) <= 4 * 2.0 ** -24 and float(whole.abs().max()) > 0
    # without the source's sums, separately: the cotangents are the same bits
    for gb, dgb in ((None, None), (torch.empty_like(lam0), None), (None, torch.empty_like(lam0))):
        l2, d2 = lam0.clone(), dlam0.clone()
        call(fwd.what0, fwd.dwhat0, l2, d2, gb, dgb)
        assert torch.equal(l2, lam) and torch.equal(d2, dlam)
        assert (gb is None or torch.equal(gb, gbar)) and (dgb is None or torch.equal(dgb, dgbar))


def test_grid_stride(gpu_device):
    c = SC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = SC.C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    dw, r, r2 = (O.band_ic(4, nx, ny, k, c[3], c[4], 1.0)[0] for k in (5, 6, 7))
    s = SC.solver('forced', c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        w = s.vorticity(s.init(dev(u0[sel]), dev(v0[sel])))
        outs.append(s.second_order_forward(w, dev(dw[sel]), 1, forcing=dev(r2[sel])).backward(dev(r[sel]), dev(r2[sel])))
    full, head, tail = outs
    for name in ('wbar', 'dwbar', 'gbar', 'dgbar'):
        x = getattr(full, name)
        assert torch.equal(x[:2], getattr(head, name)) and torch.equal(x[-2:], getattr(tail, name)) and float(x.abs().max()) > 0, name


@pytest.mark.parametrize('run', [FORCED, LINEAR], ids=SC.run_id)
def test_eager_equals_graph_replay(gpu_device, run):
    from nns import ops
    s, kw, f = setup(run)
    fwd = s.second_order_forward(f['w'], f['dw'], 2, **kw)
    lam0, dlam0 = s.init_vorticity(f['r']).what, s.init_vorticity(f['r2']).what
    work = torch.empty(ops.spec_ns_second_adjoint_workspace(run[1][2], s.nx, s.ny), dtype=torch.uint8, device='cuda')

    def call(lam, dlam, gbar, dgbar):
        ops.spec_ns_second_adjoint_(fwd.what0, fwd.dwhat0, fwd.mean, fwd.ghat, fwd.dghat, lam, dlam, gbar, dgbar, work, s.ny, s.Lx, s.Ly, s.dt,
                                    s.nu, s.drag, fwd.lin)
    eager = [lam0.clone(), dlam0.clone(), torch.empty_like(lam0), torch.empty_like(lam0)]
    call(*eager)                                                        # loads the code objects
    eager = [lam0.clone(), dlam0.clone(), torch.empty_like(lam0), torch.empty_like(lam0)]
    call(*eager)
    src = [lam0.clone(), dlam0.clone()]
    bufs = [torch.empty_like(lam0) for _ in range(4)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bufs[0].copy_(src[0])
        bufs[1].copy_(src[1])
        call(*bufs)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for got, ref in zip(bufs, eager):
        assert torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------- 4. the workspace
def test_the_call_stays_inside_its_workspace(gpu_device):
    from nns import ops
    run = FORCED
    s, kw, f = setup(run, grids=slice(0, 1))
    fwd = s.second_order_forward(f['w'], f['dw'], 2, **kw)
    need = ops.spec_ns_second_adjoint_workspace(1, s.nx, s.ny)
    assert need == max(24 * 64 * 22 * 8, ops.spec_ns_workspace(1, 64, 64))
    assert need >= ops.spec_ns_adjoint_workspace(1, 64, 64) and need >= ops.spec_ns_tangent_workspace(1, 64, 64)
    lam0, dlam0 = s.init_vorticity(f['r']).what, s.init_vorticity(f['r2']).what
    outs = []
    for pad in (0, 4096):
        buf = torch.full((need + pad,), 0xA5, dtype=torch.uint8, device='cuda')
        t = [lam0.clone(), dlam0.clone(), torch.empty_like(lam0), torch.empty_like(lam0)]
        ops.spec_ns_second_adjoint_(fwd.what0, fwd.dwhat0, fwd.mean, fwd.ghat, fwd.dghat, *t, buf[:need], s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag,
                                    fwd.lin)
        assert bool((buf[need:] == 0xA5).all())
        outs.append(t)
    for x, y in zip(*outs):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_c_entry_point_refuses_before_any_launch(gpu_device):
    from nns import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_spec_ns_second_adjoint_workspace(2, 64, 64, ctypes.byref(n)) == 0
    assert L.nns_spec_ns_second_adjoint_workspace(2, 64, 64, None) == INVALID
    t = torch.zeros(n.value, dtype=torch.uint8, device='cuda')
    what0 = torch.full((1, 2, 22, 64, 2), 3.0, device='cuda')
    lam = torch.full((2, 22, 64, 2), 5.0, device='cuda')
    dlam = torch.full((2, 22, 64, 2), 7.0, device='cuda')
    mean = torch.zeros((2, 2), device='cuda')
    P, W, A, D = t.data_ptr(), what0.data_ptr(), lam.data_ptr(), dlam.data_ptr()

    def args(dwhat0=W, dghat=None, dgbatch=0, dlam=D, nbytes=n.value, dt=0.01, gbatch=0):
        return (W, dwhat0, mean.data_ptr(), None, gbatch, dghat, dgbatch, A, dlam, None, None, P, nbytes, 2, 64, 64, TWO_PI, TWO_PI, dt, 1e-3,
                0.1, None, 1, None)
    call = L.nns_spec_ns_step_second_adjoint_f32
    assert call(*args(dwhat0=None)) == INVALID and b'dwhat0' in L.nns_last_error()
    assert call(*args(dlam=None)) == INVALID and b'dlam' in L.nns_last_error()
    assert call(*args(dt=0.0)) == INVALID
    assert call(*args(gbatch=1)) == INVALID and b'gbatch' in L.nns_last_error()
    assert call(*args(dgbatch=1)) == INVALID and b'dgbatch' in L.nns_last_error()
    assert call(*args(dghat=P, dgbatch=3)) == INVALID
    assert call(*args(nbytes=n.value - 1)) == WORKSPACE and b'nns_spec_ns_second_adjoint_workspace' in L.nns_last_error()
    torch.cuda.synchronize()
    assert bool((what0 == 3.0).all()) and bool((lam == 5.0).all()) and bool((dlam == 7.0).all())       # nothing was launched


def test_the_scalar_system_and_other_entries_are_refused(gpu_device):
    from nns.periodic import PeriodicSolver
    import inspect
    c = SC.CASES[0]
    s, kw, f = setup(FORCED)
    for more in (dict(kappa=1e-3), dict(kappa=1e-3, buoyancy=(0.0, 1.0))):
        sc = PeriodicSolver(c[0], c[1], s.dt, SC.RHO, SC.NU, drag=SC.DRAG, **more)
        with pytest.raises(NotImplementedError, match='second-order adjoint of the scalar system is not built'):
            sc.second_order_forward(f['w'], f['dw'], 1)
        with pytest.raises(NotImplementedError, match='second-order adjoint of the scalar system is not built'):
            sc.hessian_vector_product(lambda w1: w1.sum(), f['w'], f['dw'], 1)
    for name in ('second_order_forward', 'hessian_vector_product'):
        names = list(inspect.signature(getattr(PeriodicSolver, name)).parameters)
        assert 'operator' not in names and 'theta' not in names and not any(n.startswith('u0') for n in names)
    with pytest.raises(ValueError):
        s.second_order_forward(f['w'], f['dw'][:1], 1, **kw)
    run = s.second_order_forward(f['w'], f['dw'], 1, **kw)
    with pytest.raises(ValueError):
        run.backward(f['r'][:1], f['r2'][:1])
    with pytest.raises(TypeError):
        s.hessian_vector_product(lambda w1: w1, f['w'], f['dw'], 1, **kw)
