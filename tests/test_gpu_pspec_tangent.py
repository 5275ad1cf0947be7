"""GPU checks of the forward mode of the periodic solver's step (csrc/pspec_kernels.hip: nns_spec_ns_step_tangent_f32, ps_row_tan_kernel, the
TANGENT forms of ps_col_kernel; nns.periodic.PeriodicSolver.step_tangent / evolve_tangent / evolve_velocity_tangent / lyapunov_exponent)
against the float64 restatement tests/pspec_tangent_oracle.py, the existing reverse mode (the dot-product identity), analytic solutions
and its own bit identities.  Inputs fill the whole 2/3 band (tests/pspec_tangent_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_linear_cases as LC
import pspec_linear_oracle as LO
import pspec_oracle as O
import pspec_tangent_cases as TC

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = -1, -4
TWO_PI = 2 * np.pi
FORCED, LINEAR, STOCH = (('forced', TC.CASES[0]), ('linear', TC.CASES[0]), ('stochastic', TC.CASES[0]))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def cplx(t):
    w = host(t)
    return w[..., 0] + 1j * w[..., 1]


def make_solver(kind, c, dt):
    """TC.solver, and two kinds only the bit identities use: 'plain' (no drag: the unforced kernels) and 'linear-stochastic'."""
    if kind == 'plain':
        return TC.solver('forced', c, dt, drag=0.0)
    if kind == 'linear-stochastic':
        s = TC.solver('linear', c, dt)
        s.ring_forcing(*TC.LAC.ring(c), seed=TC.SEED)
        return s
    return TC.solver(kind, c, dt)


def setup(run, dg=None, grids=None, force=True):
    """(s, state, dwhat, dforcing) of a run on the device: the solver with the case's per-grid force, the state of (u0, v0), the tangent
    spectrum of dw with its (0, 0) entry set to DW_00 nx ny (the step must drop it) and the source perturbation; grids: a slice of the
    batch run alone (with its own noise ids)."""
    kind, c = run
    d = TC.inputs(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = make_solver(kind, c, d['dt'])
    if force and kind != 'plain':
        s.set_forcing(dev(pick(d['fx'])), dev(pick(d['fy'])))
    state = s.init(dev(pick(d['u0'])), dev(pick(d['v0'])))
    if s.stoch_amp is not None:
        state.noise_ids = torch.arange(c[2], dtype=torch.int32, device='cuda')[slice(None) if grids is None else grids].contiguous()
    dwhat = s.init_vorticity(dev(pick(d['dw']))).what
    dwhat[:, 0, 0, 0] = TC.DW_00 * c[0] * c[1]
    g = TC.source(c, dg)
    if g is not None:
        g = dev(g if dg == 'shared' else pick(g))
    return s, state, dwhat, g


def tangent(run, dg=None, grids=None, nsteps=TC.NSTEPS):
    s, state, dwhat, g = setup(run, dg, grids)
    s.step_tangent(state, dwhat, nsteps, dforcing=g)
    return s, state, dwhat


# ---------------------------------------------------------------------------------------------------- 1. against the float64 restatement
@pytest.mark.parametrize('run', TC.RUNS, ids=TC.run_id)
def test_tangent_against_the_oracle(gpu_device, run):
    errs = []
    for dg in (None, 'grid', 'shared'):
        s, state, dwhat = tangent(run, dg)
        errs.append(TC.rel(cplx(dwhat), TC.oracle_tangent(run, None, dg)))
    print('MEASURED %s: none %.2e grid %.2e shared %.2e' % ((TC.run_id(run),) + tuple(errs)))
    assert max(errs) <= TC.BOUND, errs


# ---------------------------------------------------------------------------------------------------- 2. the base is bitwise step
@pytest.mark.parametrize('kind', ['plain', 'forced', 'linear', 'stochastic', 'linear-stochastic'])
def test_the_base_is_bitwise_step(gpu_device, kind):
    c = TC.CASES[0]
    s, state, dwhat, g = setup((kind, c), 'grid')
    same = state.clone()
    s.step(same, TC.NSTEPS)
    before = dwhat.clone()
    out = s.step_tangent(state, dwhat, TC.NSTEPS, dforcing=g)
    assert out is dwhat and not torch.equal(dwhat, before)
    assert torch.equal(state.what, same.what) and state.steps == same.steps == TC.NSTEPS
    if s.stoch_amp is not None:
        assert torch.equal(state.clock, same.clock) and int(state.clock) == TC.NSTEPS
    else:
        assert state.clock is None and same.clock is None


@pytest.mark.parametrize('kind', ['plain', 'forced', 'linear', 'stochastic'])
def test_evolve_tangent_base_is_bitwise_evolve(gpu_device, kind):
    c = TC.CASES[0]
    d = TC.inputs(c)
    s = make_solver(kind, c, d['dt'])
    st = s.init(dev(d['u0']), dev(d['v0']))
    w, mean = s.vorticity(st), st.mean.clone()
    g = None if kind == 'plain' else s.vorticity(s.init(dev(d['fx']), dev(d['fy'])))
    kw = dict(mean=mean, forcing=g, clock=7, noise_ids=[4, 1, 9])
    ref = s.evolve(w, TC.NSTEPS, **kw)
    w_out, dw_out = s.evolve_tangent(w, dev(d['dw']), TC.NSTEPS, dforcing=dev(d['dforcing']), **kw)
    assert torch.equal(w_out, ref) and float(dw_out.abs().max()) > 0
    u, v = s.evolve_velocity(dev(d['u0']), dev(d['v0']), TC.NSTEPS, forcing=g, clock=7, noise_ids=[4, 1, 9])
    du0, dv0 = O.band_ic(c[2], c[0], c[1], 99, c[3], c[4], 1.0, mean=(0.4, 0.1))             # the perturbation's mean is dropped
    tu, tv, du, dv = s.evolve_velocity_tangent(dev(d['u0']), dev(d['v0']), dev(du0), dev(dv0), TC.NSTEPS, forcing=g, clock=7, noise_ids=[4, 1, 9])
    assert torch.equal(tu, u) and torch.equal(tv, v)
    assert float(du.abs().max()) > 0 and abs(float(du.mean())) <= 1e-6 and abs(float(dv.mean())) <= 1e-6


# ---------------------------------------------------------------------------------------------------- 3. the dot-product identity
@pytest.mark.parametrize('kind', TC.KINDS)
def test_dot_product_identity_against_the_reverse_mode(gpu_device, kind):
    """<J d, r> = <d, J^T r>: evolve_tangent against the backward of evolve, two separately written sets of kernels."""
    c = TC.CASES[0]
    d = TC.inputs(c)
    s = make_solver(kind, c, d['dt'])
    st = s.init(dev(d['u0']), dev(d['v0']))
    w, mean = s.vorticity(st).requires_grad_(True), st.mean.clone()
    g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
    dw = s.vorticity(s.init_vorticity(dev(d['dw'])))                                         # band-limited, as the step takes it
    dg = s.vorticity(s.init_vorticity(dev(d['dforcing'])))
    r = dev(d['r'])
    kw = dict(mean=mean, clock=5, noise_ids=[2, 0, 7])
    out = s.evolve(w, TC.NSTEPS, forcing=g, **kw)
    (out * r).sum().backward()
    w_out, dw_out = s.evolve_tangent(w.detach(), dw, TC.NSTEPS, forcing=g.detach(), dforcing=dg, **kw)
    assert torch.equal(w_out, out.detach())
    lhs = float((host(dw_out) * host(r)).sum())
    rhs = float((host(w.grad) * host(dw)).sum() + (host(g.grad) * host(dg)).sum())
    err = abs(lhs - rhs) / (np.linalg.norm(host(dw_out)) * np.linalg.norm(host(r)))
    print('MEASURED dot %s: <J d, r> %.9e <d, J^T r> %.9e scaled difference %.2e' % (kind, lhs, rhs, err))
    assert err <= TC.DOT_BOUND, err


# ---------------------------------------------------------------------------------------------------- 4. exact properties
@pytest.mark.parametrize('run', [FORCED, LINEAR], ids=TC.run_id)
def test_linear_in_scale_and_zero_stays_zero(gpu_device, run):
    s, state, dwhat, g = setup(run, 'grid')
    twice, zero = state.clone(), state.clone()
    d2, d0 = 2 * dwhat, torch.zeros_like(dwhat)
    s.step_tangent(state, dwhat, TC.NSTEPS, dforcing=g)
    s.step_tangent(twice, d2, TC.NSTEPS, dforcing=2 * g)
    s.step_tangent(zero, d0, TC.NSTEPS)
    assert torch.equal(d2, 2 * dwhat) and float(dwhat.abs().max()) > 0
    assert float(d0.abs().max()) == 0.0
    assert torch.equal(twice.what, state.what) and torch.equal(zero.what, state.what)


@pytest.mark.parametrize('run', [FORCED, ('forced', TC.CASES[4]), STOCH], ids=TC.run_id)
def test_a_batch_is_its_grids_and_one_call_is_chained_calls(gpu_device, run):
    s, state, dwhat = tangent(run, 'grid')
    for b in range(run[1][2]):
        _, st1, d1 = tangent(run, 'grid', grids=slice(b, b + 1))
        assert torch.equal(d1[0], dwhat[b]) and torch.equal(st1.what[0], state.what[b])
    s, st, dw, g = setup(run, 'grid')
    for _ in range(TC.NSTEPS):
        s.step_tangent(st, dw, 1, dforcing=g)
    assert torch.equal(dw, dwhat) and torch.equal(st.what, state.what) and st.steps == TC.NSTEPS


def test_grid_stride(gpu_device):
    c = TC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = TC.C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    dw = O.band_ic(4, nx, ny, 5, c[3], c[4], 1.0)[0]
    s = TC.solver('forced', c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]))
        dwhat = s.init_vorticity(dev(dw[sel])).what
        s.step_tangent(state, dwhat, 1)
        outs.append((state.what, dwhat))
    (w, t), (w01, t01), (w23, t23) = outs
    assert torch.equal(t[:2], t01) and torch.equal(t[-2:], t23) and torch.equal(w[:2], w01) and torch.equal(w[-2:], w23)
    assert float(t.abs().max()) > 0


@pytest.mark.parametrize('run', [FORCED, STOCH], ids=TC.run_id)
def test_eager_equals_graph_replay(gpu_device, run):
    s, eager, dwe, g = setup(run)
    s.step_tangent(eager, dwe, 1)                                       # grows the workspace, loads the code objects
    st, dw = eager.clone(), dwe.clone()
    s.step_tangent(eager, dwe, 2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.step_tangent(st, dw, 1)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dw, dwe) and torch.equal(st.what, eager.what)
    if s.stoch_amp is not None:
        assert int(st.clock) == int(eager.clock) == 3


# ---------------------------------------------------------------------------------------------------- 5. analytic cases
@pytest.mark.parametrize('beta', [0.0, LC.WAVE_BETA], ids=['drag', 'beta'])
def test_a_mode_on_a_base_at_rest_is_translated_damped_and_turned(gpu_device, beta):
    """Base at rest with the mean flow U: the tangent of the nonlinear term is the advection by U alone, so a single-mode perturbation is the
    exact wave of tests/pspec_linear_oracle.py: rossby_wave -- translated by U t, damped by exp(Re(lambda) t) and, with beta, turned by the
    Rossby phase -beta kx / |k|^2 t.  Shape, numbers and bound are those of the linear step's own 200-step wave test (LC.WAVE, LC.WAVE_BOUND);
    beta = 0 takes the forced kernels (nu and drag alone).  lyapunov_exponent on that base returns Re(lambda) of the mode: the growth over
    the run is the amplitude, so its error times the run's length is bounded like the amplitude's."""
    from nns.periodic import PeriodicSolver
    nx, ny, Lx, Ly, m, U, dt = LC.WAVE
    n = LC.WAVE_STEPS
    if beta:
        s = PeriodicSolver(nx, ny, dt, 1.0, LC.WAVE_NU, Lx=Lx, Ly=Ly, drag=LC.WAVE_DRAG, hyperviscosity=LC.WAVE_HYPER, hypofriction=LC.WAVE_HYPO, beta=beta)
        damping = LC.wave_damping()
    else:
        s = PeriodicSolver(nx, ny, dt, 1.0, LC.WAVE_NU, Lx=Lx, Ly=Ly, drag=LC.WAVE_DRAG)
        damping = LC.WAVE_NU * ((TWO_PI * m[0] / Lx) ** 2 + (TWO_PI * m[1] / Ly) ** 2) + LC.WAVE_DRAG
    w0 = LO.rossby_wave(nx, ny, 0.0, m, beta, damping, U, Lx, Ly)[2]
    ref, A, om = LO.rossby_wave(nx, ny, n * dt, m, beta, damping, U, Lx, Ly)[2:]
    rest = lambda: s.init_vorticity(torch.zeros((1, nx, ny), device='cuda'), mean=U)
    state, dwhat = rest(), s.init_vorticity(dev(w0)).what
    s.step_tangent(state, dwhat, n)
    assert float(state.what.abs().max()) == 0.0 and state.steps == n
    err = np.abs(host(s.vorticity(s._at_rest(dwhat)))[0] - ref).max() / A
    state, dwhat = rest(), s.init_vorticity(dev(w0)).what
    lam = float(s.lyapunov_exponent(state, dwhat, n, 50)[0])
    print('mode %s on U %s, beta %g, %d steps: amplitude %.4f, phase %.3f rad; max error / amplitude %.2e; exponent %.9f, Re(lambda) %.9f'
          % (m, U, beta, n, A, om * n * dt, err, lam, -damping))
    assert err <= LC.WAVE_BOUND, err
    assert abs(lam + damping) * n * dt <= LC.WAVE_BOUND, (lam, -damping)
    assert abs(float(s.diagnostics(s._at_rest(dwhat)).energy[0]) - 1.0) <= 1e-6          # left at unit energy


# ---------------------------------------------------------------------------------------------------- 6. the workspace
def test_the_call_stays_inside_its_workspace(gpu_device):
    from nns import ops
    run = FORCED
    _, ref_state, ref = tangent(run, 'grid', grids=slice(0, 1), nsteps=2)
    s, state, dwhat, g = setup(run, 'grid', grids=slice(0, 1))
    need = ops.spec_ns_tangent_workspace(1, s.nx, s.ny)
    assert need == max(12 * 64 * 22 * 8, ops.spec_ns_workspace(1, 64, 64)) and need >= ops.spec_ns_workspace(1, 64, 64)
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    state.work = buf[:need]
    s.step_tangent(state, dwhat, 2, dforcing=g)
    assert state.work.data_ptr() == buf.data_ptr()
    assert bool((buf[need:] == 0xA5).all())
    assert torch.equal(dwhat, ref) and torch.equal(state.what, ref_state.what)


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_c_entry_point_refuses_before_any_launch(gpu_device):
    from nns import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_spec_ns_tangent_workspace(2, 64, 64, ctypes.byref(n)) == 0
    assert L.nns_spec_ns_tangent_workspace(2, 64, 64, None) == INVALID
    t = torch.zeros(n.value, dtype=torch.uint8, device='cuda')
    what = torch.full((2, 22, 64, 2), 3.0, device='cuda')
    dwhat = torch.full((2, 22, 64, 2), 5.0, device='cuda')
    mean = torch.zeros((2, 2), device='cuda')
    P, W, D = t.data_ptr(), what.data_ptr(), dwhat.data_ptr()

    def args(dwhat=D, dghat=None, dgbatch=0, nbytes=n.value, amp=None, clock=None, ids=None):
        return (W, dwhat, mean.data_ptr(), None, 0, dghat, dgbatch, P, nbytes, 2, 64, 64, TWO_PI, TWO_PI, 0.01, 1e-3, 0.1, None, amp, 0,
                clock, ids, 1, None)
    call = L.nns_spec_ns_step_tangent_f32
    assert call(*args(dwhat=None)) == INVALID and b'dwhat' in L.nns_last_error()
    assert call(*args(dgbatch=1)) == INVALID and b'dgbatch' in L.nns_last_error()
    assert call(*args(dghat=P, dgbatch=0)) == INVALID
    assert call(*args(dghat=P, dgbatch=3)) == INVALID
    assert call(*args(nbytes=n.value - 1)) == WORKSPACE and b'nns_spec_ns_tangent_workspace' in L.nns_last_error()
    assert call(*args(amp=P)) == INVALID
    assert call(*args(amp=P, clock=P)) == INVALID
    torch.cuda.synchronize()
    assert bool((what == 3.0).all()) and bool((dwhat == 5.0).all())       # nothing was launched


def test_a_state_with_a_scalar_is_refused_and_one_without_is_stepped(gpu_device):
    from nns.periodic import PeriodicSolver
    c = TC.CASES[0]
    d = TC.inputs(c)
    for kw in (dict(kappa=1e-3), dict(kappa=1e-3, buoyancy=(0.0, 1.0))):
        s = PeriodicSolver(c[0], c[1], d['dt'], TC.RHO, TC.NU, drag=TC.DRAG, **kw)
        state = s.init(dev(d['u0']), dev(d['v0']), dev(d['r']))
        dwhat = s.init_vorticity(dev(d['dw'])).what
        for call in (lambda: s.step_tangent(state, dwhat, 1), lambda: s.lyapunov_exponent(state, dwhat, 2, 1)):
            with pytest.raises(NotImplementedError, match='tangent of the scalar system is not built'):
                call()
        free = s.init(dev(d['u0']), dev(d['v0']))
        s.step_tangent(free, dwhat, 2)
        plain = PeriodicSolver(c[0], c[1], d['dt'], TC.RHO, TC.NU, drag=TC.DRAG)
        st, dw = plain.init(dev(d['u0']), dev(d['v0'])), plain.init_vorticity(dev(d['dw'])).what
        plain.step_tangent(st, dw, 2)
        assert torch.equal(dw, dwhat) and torch.equal(st.what, free.what)
    with pytest.raises(ValueError):
        plain.step_tangent(st, dw[:1], 1)
    with pytest.raises(TypeError):
        plain.step_tangent(st, None, 1)
