"""GPU checks of the forward mode of the periodic solver's step with a scalar (csrc/pspec_kernels.hip: nns_spec_ns_step_scalar_tangent_f32,
ps_row_tan_scalar_kernel, the PsScalar + PsTangent + PsTangentScalar forms of ps_col_kernel; nns.periodic.PeriodicSolver.step_tangent_scalar
/ evolve_tangent_scalar / evolve_velocity_tangent_scalar / lyapunov_exponent_scalar) against the float64 restatement
tests/pspec_scalar_tangent_oracle.py, the existing reverse mode (the dot-product identity), the flow's tangent step, an eigenmode of the
linear problem at rest and its own bit identities.  Inputs fill the whole 2/3 band (tests/pspec_scalar_tangent_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_oracle as O
import pspec_scalar_tangent_cases as TC

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = -1, -4
TWO_PI = 2 * np.pi
C0 = TC.CASES[0]
PASSIVE, BUOYANT, LINEAR, STOCH = (('passive', C0), ('buoyant', C0), ('buoyant-linear', C0), ('buoyant-stochastic', C0))
# amplitude errors of the eigenmode from rest after 200 steps (dw, dtheta; max error / amplitude) and |exponent - Re lambda| x run length for
# scalar_weight 1 and 4, measured on the MI355X; EIGEN_BOUND is 3-7x the worst of them, rounded
EIGEN_MEASURED = (6.89e-7, 4.04e-7, 5.32e-7, 5.10e-8)
EIGEN_BOUND = 3e-6        # 4.4x the worst (dw's amplitude)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def cplx(t):
    w = host(t)
    return w[..., 0] + 1j * w[..., 1]


def make_solver(kind, c, dt):
    """TC.solver, and two kinds only the bit identities use: 'buoyant-forced-off' (no drag: with no force the unforced kernels) and
    'linear-stochastic'."""
    if kind == 'buoyant-forced-off':
        return TC.solver('buoyant', c, dt, drag=0.0)
    if kind == 'linear-stochastic':
        s = TC.solver('buoyant-linear', c, dt)
        s.ring_forcing(*TC.LAC.ring(c), seed=TC.SEED)
        return s
    return TC.solver(kind, c, dt)


def scalar_spectrum(s, theta):
    """theta^ of a field as the state holds it."""
    from nns import ops
    B = theta.shape[0]
    that = torch.empty((B, s.my1, s.nx, 2), dtype=torch.float32, device='cuda')
    return ops.spec_ns_scalar_init(theta.contiguous(), that, s._work(ops.spec_ns_scalar_workspace, B, that.device))


def setup(run, dg=None, grids=None):
    """(s, state, dwhat, dthat, dforcing) of a run on the device: the solver with the case's per-grid force (none for 'buoyant-forced-off'),
    the state of (u0, v0, theta0), the tangent spectra of (dw, dtheta), dwhat's (0, 0) entry set to DW_00 nx ny (the step must drop it),
    and the source perturbation; grids: a slice of the batch run alone (with its own noise ids)."""
    kind, c = run
    d = TC.inputs(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = make_solver(kind, c, d['dt'])
    if kind != 'buoyant-forced-off':
        s.set_forcing(dev(pick(d['fx'])), dev(pick(d['fy'])))
    state = s.init(dev(pick(d['u0'])), dev(pick(d['v0'])), dev(pick(d['theta0'])))
    if s.stoch_amp is not None:
        state.noise_ids = torch.arange(c[2], dtype=torch.int32, device='cuda')[slice(None) if grids is None else grids].contiguous()
    dwhat = s.init_vorticity(dev(pick(d['dw']))).what
    dwhat[:, 0, 0, 0] = TC.DW_00 * c[0] * c[1]
    dthat = scalar_spectrum(s, dev(pick(d['dtheta'])))
    g = TC.source(c, dg)
    if g is not None:
        g = dev(g if dg == 'shared' else pick(g))
    return s, state, dwhat, dthat, g


def tangent(run, dg=None, grids=None, nsteps=None):
    s, state, dwhat, dthat, g = setup(run, dg, grids)
    nsteps = TC.steps(run) if nsteps is None else nsteps
    s.step_tangent_scalar(state, dwhat, dthat, nsteps, dforcing=g)
    return s, state, dwhat, dthat


# ---------------------------------------------------------------------------------------------------- 1. against the float64 restatement
@pytest.mark.parametrize('run', TC.RUNS, ids=TC.run_id)
def test_tangent_against_the_oracle(gpu_device, run):
    errs = []
    for dg in (None, 'grid', 'shared'):
        s, state, dwhat, dthat = tangent(run, dg)
        ref = TC.oracle_tangent(run, None, dg)
        errs.append((TC.rel(cplx(dwhat), ref[0]), TC.rel(cplx(dthat), ref[1])))
    print('MEASURED %s: dw none %.2e grid %.2e shared %.2e; dtheta none %.2e grid %.2e shared %.2e'
          % ((TC.run_id(run),) + tuple(e[0] for e in errs) + tuple(e[1] for e in errs)))
    assert max(e[0] for e in errs) <= TC.BOUND_W and max(e[1] for e in errs) <= TC.BOUND_T, errs


def test_grid_stride(gpu_device):
    c = TC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = TC.C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    th0, dw, dth = (O.band_ic(4, nx, ny, seed, c[3], c[4], 1.0)[0] for seed in (3, 5, 6))
    s = TC.solver('buoyant', c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]), dev(th0[sel]))
        dwhat, dthat = s.init_vorticity(dev(dw[sel])).what, scalar_spectrum(s, dev(dth[sel] + 0.3))
        s.step_tangent_scalar(state, dwhat, dthat, 1)
        outs.append((state.what, state.that, dwhat, dthat))
    full, first, last = outs
    for a, b01, b23 in zip(full, first, last):
        assert torch.equal(a[:2], b01) and torch.equal(a[-2:], b23)
    assert float(full[2].abs().max()) > 0 and float(full[3].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 2. the base is bitwise step
@pytest.mark.parametrize('kind', ['passive', 'buoyant', 'buoyant-forced-off', 'buoyant-linear', 'buoyant-stochastic', 'linear-stochastic'])
def test_the_base_is_bitwise_step(gpu_device, kind):
    s, state, dwhat, dthat, g = setup((kind, C0), 'grid')
    same = state.clone()
    s.step(same, TC.NSTEPS)
    bw, bt = dwhat.clone(), dthat.clone()
    out = s.step_tangent_scalar(state, dwhat, dthat, TC.NSTEPS, dforcing=g)
    assert out[0] is dwhat and out[1] is dthat and not torch.equal(dwhat, bw) and not torch.equal(dthat, bt)
    assert torch.equal(state.what, same.what) and torch.equal(state.that, same.that) and state.steps == same.steps == TC.NSTEPS
    if s.stoch_amp is not None:
        assert torch.equal(state.clock, same.clock) and int(state.clock) == TC.NSTEPS
    else:
        assert state.clock is None and same.clock is None


@pytest.mark.parametrize('kind', ['passive', 'buoyant', 'buoyant-linear', 'buoyant-stochastic'])
def test_evolve_tangent_scalar_base_is_bitwise_evolve(gpu_device, kind):
    c = C0
    d = TC.inputs(c)
    s = make_solver(kind, c, d['dt'])
    st = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']))
    w, theta, mean = s.vorticity(st), s.scalar(st), st.mean.clone()
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy'])))
    kw = dict(mean=mean, forcing=g, clock=7, noise_ids=[4, 1, 9])
    rw, rt = s.evolve(w, TC.NSTEPS, theta=theta, **kw)
    out = s.evolve_tangent_scalar(w, theta, dev(d['dw']), dev(d['dtheta']), TC.NSTEPS, dforcing=dev(d['dforcing']), **kw)
    assert torch.equal(out[0], rw) and torch.equal(out[1], rt) and float(out[2].abs().max()) > 0 and float(out[3].abs().max()) > 0
    kw = dict(forcing=g, clock=7, noise_ids=[4, 1, 9])
    u, v, th = s.evolve_velocity(dev(d['u0']), dev(d['v0']), TC.NSTEPS, theta0=dev(d['theta0']), **kw)
    du0, dv0 = O.band_ic(c[2], c[0], c[1], 99, c[3], c[4], 1.0, mean=(0.4, 0.1))             # the perturbation's mean is dropped
    out = s.evolve_velocity_tangent_scalar(dev(d['u0']), dev(d['v0']), dev(d['theta0']), dev(du0), dev(dv0), dev(d['dtheta']), TC.NSTEPS, **kw)
    assert torch.equal(out[0], u) and torch.equal(out[1], v) and torch.equal(out[2], th)
    assert float(out[3].abs().max()) > 0 and abs(float(out[3].mean())) <= 1e-6 and abs(float(out[4].mean())) <= 1e-6
    assert abs(float(out[5].mean()) - TC.DTHETA_MEAN) <= 1e-6


# ---------------------------------------------------------------------------------------------------- 3. without buoyancy: the flow's tangent
@pytest.mark.parametrize('kind', ['passive', 'passive-linear'])
def test_without_buoyancy_dwhat_is_bitwise_step_tangent(gpu_device, kind):
    from nns.periodic import PeriodicState
    s, state, dwhat, dthat, g = setup((kind, C0), 'grid')
    flow = PeriodicState(state.what.clone(), state.mean.clone(), torch.empty_like(state.work))         # a scalar-free clone of the flow
    dflow = dwhat.clone()
    s.step_tangent(flow, dflow, TC.NSTEPS, dforcing=g)
    s.step_tangent_scalar(state, dwhat, dthat, TC.NSTEPS, dforcing=g)
    assert torch.equal(dwhat, dflow) and torch.equal(state.what, flow.what) and float(dwhat.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 4. the dot-product identity
@pytest.mark.parametrize('kind', TC.DOT_KINDS)
def test_dot_product_identity_against_the_reverse_mode(gpu_device, kind):
    """<J d, r> = <d, J^T r>: evolve_tangent_scalar against the backward of evolve with theta, two separately written sets of kernels."""
    c = C0
    d = TC.inputs(c)
    s = make_solver(kind, c, d['dt'])
    st = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']))
    w, theta, mean = s.vorticity(st).requires_grad_(True), s.scalar(st).requires_grad_(True), st.mean.clone()
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    band = lambda a: s.vorticity(s.init_vorticity(dev(a)))                                   # band-limited, as the step takes it
    dw, dg = band(d['dw']), band(d['dforcing'])
    dth = s.scalar(s.init(dev(d['u0']), dev(d['v0']), dev(d['dtheta'])))
    rw, rt = dev(d['rw']), dev(d['rt'])
    kw = dict(mean=mean, clock=5, noise_ids=[2, 0, 7])
    ow, ot = s.evolve(w, TC.NSTEPS, theta=theta, forcing=g, **kw)
    ((ow * rw).sum() + (ot * rt).sum()).backward()
    tw, tt, jw, jt = s.evolve_tangent_scalar(w.detach(), theta.detach(), dw, dth, TC.NSTEPS, forcing=g.detach(), dforcing=dg, **kw)
    assert torch.equal(tw, ow.detach()) and torch.equal(tt, ot.detach())
    dot = lambda a, b: float((host(a) * host(b)).sum())
    lhs = dot(jw, rw) + dot(jt, rt)
    rhs = dot(w.grad, dw) + dot(theta.grad, dth) + dot(g.grad, dg)
    norm = lambda *a: float(np.sqrt(sum(np.linalg.norm(host(x)) ** 2 for x in a)))
    err = abs(lhs - rhs) / (norm(jw, jt) * norm(rw, rt))
    print('MEASURED dot %s: <J d, r> %.9e <d, J^T r> %.9e scaled difference %.2e' % (kind, lhs, rhs, err))
    assert err <= TC.DOT_BOUND, err


# ---------------------------------------------------------------------------------------------------- 5. exact properties
@pytest.mark.parametrize('run', [BUOYANT, LINEAR], ids=TC.run_id)
def test_linear_in_scale_and_zero_stays_zero(gpu_device, run):
    s, state, dwhat, dthat, g = setup(run, 'grid')
    twice, zero = state.clone(), state.clone()
    w2, t2, w0, t0 = 2 * dwhat, 2 * dthat, torch.zeros_like(dwhat), torch.zeros_like(dthat)
    s.step_tangent_scalar(state, dwhat, dthat, TC.NSTEPS, dforcing=g)
    s.step_tangent_scalar(twice, w2, t2, TC.NSTEPS, dforcing=2 * g)
    s.step_tangent_scalar(zero, w0, t0, TC.NSTEPS)
    assert torch.equal(w2, 2 * dwhat) and torch.equal(t2, 2 * dthat) and float(dwhat.abs().max()) > 0 and float(dthat.abs().max()) > 0
    assert float(w0.abs().max()) == 0.0 and float(t0.abs().max()) == 0.0
    for other in (twice, zero):
        assert torch.equal(other.what, state.what) and torch.equal(other.that, state.that)


@pytest.mark.parametrize('run', [BUOYANT, ('buoyant', TC.CASES[2]), STOCH], ids=TC.run_id)
def test_a_batch_is_its_grids_and_one_call_is_chained_calls(gpu_device, run):
    s, state, dwhat, dthat = tangent(run, 'grid')
    for b in range(run[1][2]):
        _, st1, w1, t1 = tangent(run, 'grid', grids=slice(b, b + 1))
        assert torch.equal(w1[0], dwhat[b]) and torch.equal(t1[0], dthat[b])
        assert torch.equal(st1.what[0], state.what[b]) and torch.equal(st1.that[0], state.that[b])
    s, st, dw, dth, g = setup(run, 'grid')
    for _ in range(TC.steps(run)):
        s.step_tangent_scalar(st, dw, dth, 1, dforcing=g)
    assert torch.equal(dw, dwhat) and torch.equal(dth, dthat) and torch.equal(st.what, state.what) and torch.equal(st.that, state.that)
    assert st.steps == TC.steps(run)


@pytest.mark.parametrize('run', [BUOYANT, STOCH], ids=TC.run_id)
def test_eager_equals_graph_replay(gpu_device, run):
    s, eager, dwe, dte, g = setup(run)
    s.step_tangent_scalar(eager, dwe, dte, 1)                           # grows the workspace, loads the code objects
    st, dw, dth = eager.clone(), dwe.clone(), dte.clone()
    s.step_tangent_scalar(eager, dwe, dte, 2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.step_tangent_scalar(st, dw, dth, 1)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dw, dwe) and torch.equal(dth, dte) and torch.equal(st.what, eager.what) and torch.equal(st.that, eager.that)
    if s.stoch_amp is not None:
        assert int(st.clock) == int(eager.clock) == 3


@pytest.mark.parametrize('run', [PASSIVE, BUOYANT], ids=TC.run_id)
def test_the_mean_of_dtheta_stays_and_a_mean_of_dw_is_dropped(gpu_device, run):
    s, state, dwhat, dthat, g = setup(run, 'grid')
    mean_in = dthat[:, 0, 0].clone()
    assert float(mean_in[:, 0].abs().min()) > 0 and float(dwhat[:, 0, 0, 0].abs().min()) > 0
    clean_state, clean = state.clone(), dwhat.clone()
    clean[:, 0, 0] = 0.0
    ct = dthat.clone()
    s.step_tangent_scalar(state, dwhat, dthat, TC.NSTEPS, dforcing=g)
    s.step_tangent_scalar(clean_state, clean, ct, TC.NSTEPS, dforcing=g)
    assert torch.equal(dthat[:, 0, 0], mean_in)                        # as it went in, bit for bit
    assert float(dwhat[:, 0, 0].abs().max()) == 0.0 and torch.equal(dwhat, clean) and torch.equal(dthat, ct)


# ---------------------------------------------------------------------------------------------------- 6. the eigenmode from rest
def test_an_eigenmode_from_rest_grows_at_its_rate(gpu_device):
    """Base at rest with the mean flow U: the tangent is the 2 x 2 linear problem per mode, whose growing eigenmode (convection, b . G < 0)
    must come out translated by U t and grown by exp(Re lambda t), both fields (tests/pspec_scalar_tangent_cases.py: eigenmode; the
    restatement's own error is 4.9e-10).  lyapunov_exponent_scalar on that base returns Re lambda whatever the weight of the scalar: the
    growth over the run is the amplitude, so its error times the run's length is bounded like the amplitude's."""
    from nns.periodic import PeriodicSolver
    p = TC.EIGEN
    n = p['nsteps']
    s = PeriodicSolver(p['nx'], p['ny'], p['dt'], 1.0, p['nu'], drag=p['drag'], kappa=p['kappa'], scalar_gradient=p['G'], buoyancy=p['b'])
    dw0, dt0, lam = TC.eigenmode(0.0)[:3]
    rw, rt, _, aw, at = TC.eigenmode(n * p['dt'])
    zero = torch.zeros((1, p['nx'], p['ny']), device='cuda')

    def rest():
        state = s.init_vorticity(zero, mean=p['U'])
        state.that = scalar_spectrum(s, zero)
        return state, s.init_vorticity(dev(dw0[None])).what, scalar_spectrum(s, dev(dt0[None]))
    state, dwhat, dthat = rest()
    s.step_tangent_scalar(state, dwhat, dthat, n)
    assert float(state.what.abs().max()) == 0.0 and state.steps == n
    base = state.that.clone()                                           # the base's theta stays uniform: its mean falls by t G . U, its fluctuation stays zero
    base[:, 0, 0] = 0.0
    assert float(base.abs().max()) == 0.0
    out = s._at_rest(dwhat, state.work)
    out.that = dthat
    ew = np.abs(host(s.vorticity(out))[0] - rw).max() / aw
    et = np.abs(host(s.scalar(out))[0] - rt).max() / at
    figures = [ew, et]
    for weight in (1.0, 4.0):
        state, dwhat, dthat = rest()
        got = float(s.lyapunov_exponent_scalar(state, dwhat, dthat, n, 50, scalar_weight=weight)[0])
        figures.append(abs(got - lam) * n * p['dt'])
        print('scalar_weight %g: exponent %.9f, Re lambda %.9f' % (weight, got, lam))
    print('MEASURED eigenmode %s on U %s, %d steps: growth %.4f; max error / amplitude dw %.2e dtheta %.2e; exponent error x T %.2e %.2e'
          % ((p['m'], p['U'], n, aw) + tuple(figures)))
    assert max(figures) <= EIGEN_BOUND, figures


# ---------------------------------------------------------------------------------------------------- 7. the workspace and the refusals
def test_the_call_stays_inside_its_workspace(gpu_device):
    from nns import ops
    run = BUOYANT
    _, ref_state, rw, rt = tangent(run, 'grid', grids=slice(0, 1), nsteps=2)
    s, state, dwhat, dthat, g = setup(run, 'grid', grids=slice(0, 1))
    need = ops.spec_ns_scalar_tangent_workspace(1, s.nx, s.ny)
    assert need == max(20 * 64 * 22 * 8, ops.spec_ns_workspace(1, 64, 64))
    assert need >= ops.spec_ns_scalar_workspace(1, 64, 64) and need >= ops.spec_ns_tangent_workspace(1, 64, 64)
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    state.work = buf[:need]
    s.step_tangent_scalar(state, dwhat, dthat, 2, dforcing=g)
    assert state.work.data_ptr() == buf.data_ptr()
    assert bool((buf[need:] == 0xA5).all())
    assert torch.equal(dwhat, rw) and torch.equal(dthat, rt) and torch.equal(state.what, ref_state.what) and torch.equal(state.that, ref_state.that)


def test_c_entry_point_refuses_before_any_launch(gpu_device):
    from nns import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_spec_ns_scalar_tangent_workspace(2, 64, 64, ctypes.byref(n)) == 0
    assert L.nns_spec_ns_scalar_tangent_workspace(2, 64, 64, None) == INVALID
    t = torch.zeros(n.value, dtype=torch.uint8, device='cuda')
    fields = [torch.full((2, 22, 64, 2), v, device='cuda') for v in (3.0, 4.0, 5.0, 6.0)]
    mean = torch.zeros((2, 2), device='cuda')
    P = t.data_ptr()
    W, T, DW, DT = (f.data_ptr() for f in fields)

    def args(that=T, dwhat=DW, dthat=DT, dghat=None, dgbatch=0, nbytes=n.value, amp=None, clock=None, ids=None, kappa=1e-3):
        return (W, that, dwhat, dthat, mean.data_ptr(), None, 0, dghat, dgbatch, P, nbytes, 2, 64, 64, TWO_PI, TWO_PI, 0.01, 1e-3, 0.1, kappa,
                0.2, -0.1, 0.0, 1.0, None, amp, 0, clock, ids, 1, None)
    call = L.nns_spec_ns_step_scalar_tangent_f32
    for name in ('that', 'dwhat', 'dthat'):
        assert call(*args(**{name: None})) == INVALID and name.encode() in L.nns_last_error()
    assert call(*args(dgbatch=1)) == INVALID and b'dgbatch' in L.nns_last_error()
    assert call(*args(dghat=P, dgbatch=0)) == INVALID
    assert call(*args(dghat=P, dgbatch=3)) == INVALID
    assert call(*args(nbytes=n.value - 1)) == WORKSPACE and b'nns_spec_ns_scalar_tangent_workspace' in L.nns_last_error()
    assert call(*args(amp=P)) == INVALID
    assert call(*args(kappa=-1.0)) == INVALID                          # the forward entry's own refusals
    torch.cuda.synchronize()
    assert all(bool((f == v).all()) for f, v in zip(fields, (3.0, 4.0, 5.0, 6.0)))      # nothing was launched


def test_a_state_without_a_scalar_is_refused(gpu_device):
    from nns.periodic import PeriodicSolver
    c = C0
    d = TC.inputs(c)
    s = PeriodicSolver(c[0], c[1], d['dt'], TC.RHO, TC.NU, drag=TC.DRAG, kappa=TC.KAPPA, buoyancy=TC.UNSTABLE)
    free, state = s.init(dev(d['u0']), dev(d['v0'])), s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']))
    dwhat, dthat = s.init_vorticity(dev(d['dw'])).what, scalar_spectrum(s, dev(d['dtheta']))
    for call in (lambda: s.step_tangent_scalar(free, dwhat, dthat, 1), lambda: s.lyapunov_exponent_scalar(free, dwhat, dthat, 2, 1)):
        with pytest.raises(ValueError, match='carries no scalar'):
            call()
    with pytest.raises(ValueError):
        s.step_tangent_scalar(state, dwhat, dthat[:1], 1)
    with pytest.raises(TypeError):
        s.step_tangent_scalar(state, dwhat, None, 1)
    with pytest.raises(ValueError, match='scalar_weight'):
        s.lyapunov_exponent_scalar(state, dwhat, dthat, 2, 1, scalar_weight=0.0)
    with pytest.raises(NotImplementedError, match='tangent of the scalar system is not built'):
        s.step_tangents(state, s.init_tangents(dev(d['dw'])[None]), 1)
    assert state.steps == 0
