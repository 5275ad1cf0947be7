"""GPU checks of K tangents on one base and of the Lyapunov spectrum of the periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_tangents_f32, ps_row_tans_kernel, the TANGENTS forms of ps_col_kernel, ps_tangent_gram_kernel, ps_tangent_combine_kernel;
nns.periodic.PeriodicSolver.init_tangents / step_tangents / tangent_gram / orthonormalize_tangents / lyapunov_spectrum) against
step_tangent bit for bit, the float64 restatement tests/pspec_lyapunov_oracle.py and analytic exponents (tests/pspec_lyapunov_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_linear_cases as LIN
import pspec_lyapunov_cases as LC
import pspec_lyapunov_oracle as LY
import pspec_tangent_cases as TC

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = -1, -4
TWO_PI = 2 * np.pi
FORCED, LINEAR, STOCH = LC.SPECTRUM_RUNS
K3 = LC.K_BITWISE


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def make_solver(kind, c, dt):
    """TC.solver, and two kinds only the bit identities use: 'plain' (no drag: the unforced kernels) and 'linear-stochastic'."""
    if kind == 'plain':
        return TC.solver('forced', c, dt, drag=0.0)
    if kind == 'linear-stochastic':
        s = TC.solver('linear', c, dt)
        s.ring_forcing(*TC.LAC.ring(c), seed=TC.SEED)
        return s
    return TC.solver(kind, c, dt)


def setup(run, K, grids=None, fields=None):
    """(s, state, dwhat) of a run on the device: the solver with the case's per-grid force, the state of (u0, v0) and the K tangent spectra;
    grids: a slice of the batch run alone (with its own noise ids); fields: other perturbations than LC.tangent_fields."""
    kind, c = run
    d = TC.inputs(c)
    pick = (lambda a: a) if grids is None else (lambda a: a[grids])
    s = make_solver(kind, c, d['dt'])
    if kind != 'plain':
        s.set_forcing(dev(pick(d['fx'])), dev(pick(d['fy'])))
    state = s.init(dev(pick(d['u0'])), dev(pick(d['v0'])))
    if s.stoch_amp is not None:
        state.noise_ids = torch.arange(c[2], dtype=torch.int32, device='cuda')[slice(None) if grids is None else grids].contiguous()
    f = LC.tangent_fields(c, K) if fields is None else fields
    dwhat = s.init_tangents(dev(f[:, slice(None) if grids is None else grids]))
    return s, state, dwhat


def singles(s, state, dwhat, nsteps, members=None):
    """What step_tangent gives for each member alone from a clone of the state: [(k, state_k, dwhat_k)]."""
    out = []
    for k in range(dwhat.shape[0]) if members is None else members:
        st, dk = state.clone(), dwhat[k].clone()
        s.step_tangent(st, dk, nsteps)
        out.append((k, st, dk))
    return out


def expand(s, spec):
    """complex128 rfft2-layout spectra [..., nx, nh] of compact float32 spectra [..., my1, nx, 2] (zero beyond the kept y-wavenumbers)."""
    z = host(spec)
    z = np.swapaxes(z[..., 0] + 1j * z[..., 1], -1, -2)
    out = np.zeros(z.shape[:-1] + (s.ny // 2 + 1,), dtype=np.complex128)
    out[..., :s.my1] = z
    return out


def oracle_of(s, kind='forced', c=None, dt=None):
    c = TC.CASES[0] if c is None else c
    return LY.Lyapunov(TC.scheme(kind, c, TC.inputs(c)['dt'] if dt is None else dt))


# ---------------------------------------------------------------------------------------------------- 1. bitwise against step_tangent
BITWISE_RUNS = TC.RUNS + [('plain', TC.CASES[0]), ('linear-stochastic', TC.CASES[0])]


@pytest.mark.parametrize('run', BITWISE_RUNS, ids=TC.run_id)
def test_base_and_every_member_are_bitwise_step_and_step_tangent(gpu_device, run):
    s, state, dwhat = setup(run, K3)
    same = state.clone()
    s.step(same, LC.NSTEPS_BITWISE)
    ref = singles(s, state, dwhat, LC.NSTEPS_BITWISE)
    before = dwhat.clone()
    out = s.step_tangents(state, dwhat, LC.NSTEPS_BITWISE)
    assert out is dwhat and not torch.equal(dwhat, before)
    assert torch.equal(state.what, same.what) and state.steps == same.steps == LC.NSTEPS_BITWISE
    if s.stoch_amp is not None:
        assert torch.equal(state.clock, same.clock) and int(state.clock) == LC.NSTEPS_BITWISE
    for k, st, dk in ref:
        assert torch.equal(st.what, state.what)
        assert torch.equal(dwhat[k], dk), 'member %d' % k


# ---------------------------------------------------------------------------------------------------- 2. K and neighbours do not matter
def test_a_member_does_not_depend_on_K(gpu_device):
    s, state, dwhat = setup(FORCED, 5)
    one_state, one = state.clone(), dwhat[3:4].clone()
    s.step_tangents(state, dwhat, 2)
    s.step_tangents(one_state, one, 2)
    assert torch.equal(one[0], dwhat[3]) and torch.equal(one_state.what, state.what)


def test_K_32_first_and_last_member(gpu_device):
    c = (64, 64, 1) + TC.CASES[0][3:]
    s, state, dwhat = setup(('forced', c), 32)
    ref = singles(s, state, dwhat, 1, members=(0, 31))
    s.step_tangents(state, dwhat, 1)
    for k, st, dk in ref:
        assert torch.equal(dwhat[k], dk) and torch.equal(st.what, state.what)
    assert float(dwhat[31].abs().max()) > 0


@pytest.mark.parametrize('run', [FORCED, STOCH], ids=TC.run_id)
def test_a_batch_is_its_grids_and_one_call_is_chained_calls(gpu_device, run):
    s, state, dwhat = setup(run, K3)
    s.step_tangents(state, dwhat, 3)
    for b in range(run[1][2]):
        s1, st1, d1 = setup(run, K3, grids=slice(b, b + 1))
        s1.step_tangents(st1, d1, 3)
        assert torch.equal(d1[:, 0], dwhat[:, b]) and torch.equal(st1.what[0], state.what[b])
    s, st, dw = setup(run, K3)
    for _ in range(3):
        s.step_tangents(st, dw, 1)
    assert torch.equal(dw, dwhat) and torch.equal(st.what, state.what) and st.steps == 3


def test_grid_stride(gpu_device):
    c = LC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = TC.C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    dw = np.stack([TC.O.band_ic(4, nx, ny, 5 + 100 * k, c[3], c[4], 1.0)[0] for k in range(2)])
    s = TC.solver('forced', c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]))
        dwhat = s.init_tangents(dev(dw[:, sel]))
        s.step_tangents(state, dwhat, 1)
        outs.append((state.what, dwhat))
    (w, t), (w01, t01), (w23, t23) = outs
    assert torch.equal(t[:, :2], t01) and torch.equal(t[:, -2:], t23) and torch.equal(w[:2], w01) and torch.equal(w[-2:], w23)
    assert float(t[1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 3. eager equals graph replay
@pytest.mark.parametrize('run', [FORCED, STOCH], ids=TC.run_id)
def test_eager_equals_graph_replay(gpu_device, run):
    s, eager, dwe = setup(run, 2)
    s.step_tangents(eager, dwe, 1)                                      # grows the workspace, loads the code objects
    st, dw = eager.clone(), dwe.clone()
    s.step_tangents(eager, dwe, 2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.step_tangents(st, dw, 1)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dw, dwe) and torch.equal(st.what, eager.what)
    if s.stoch_amp is not None:
        assert int(st.clock) == int(eager.clock) == 3


# ---------------------------------------------------------------------------------------------------- 4. the workspace
def test_the_call_stays_inside_its_workspace(gpu_device):
    from nns import ops
    s, ref_state, ref = setup(FORCED, K3, grids=slice(0, 1))
    s.step_tangents(ref_state, ref, 2)
    s, state, dwhat = setup(FORCED, K3, grids=slice(0, 1))
    need = ops.spec_ns_tangents_workspace(1, K3, s.nx, s.ny)
    assert need == max((6 + 6 * 3) * 64 * 22 * 8, ops.spec_ns_workspace(1, 64, 64)) and need >= ops.spec_ns_workspace(1, 64, 64)
    assert ops.spec_ns_tangents_workspace(1, 1, 64, 64) == ops.spec_ns_tangent_workspace(1, 64, 64)
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    state.work = buf[:need]
    s.step_tangents(state, dwhat, 2)
    assert state.work.data_ptr() == buf.data_ptr()
    assert bool((buf[need:] == 0xA5).all())
    assert torch.equal(dwhat, ref) and torch.equal(state.what, ref_state.what)


# ---------------------------------------------------------------------------------------------------- 5. the C entries refuse before any launch
def test_c_entry_points_refuse_before_any_launch(gpu_device):
    from nns import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_spec_ns_tangents_workspace(2, 3, 64, 64, ctypes.byref(n)) == 0
    assert L.nns_spec_ns_tangents_workspace(2, 3, 64, 64, None) == INVALID
    assert L.nns_spec_ns_tangents_workspace(2, 0, 64, 64, ctypes.byref(n)) == INVALID
    assert L.nns_spec_ns_tangents_workspace(2, 33, 64, 64, ctypes.byref(n)) == INVALID and b'ntan' in L.nns_last_error()
    t = torch.zeros(n.value, dtype=torch.uint8, device='cuda')
    what = torch.full((2, 22, 64, 2), 3.0, device='cuda')
    dwhat = torch.full((3, 2, 22, 64, 2), 5.0, device='cuda')
    mean = torch.zeros((2, 2), device='cuda')
    gram = torch.full((2, 3, 3), 7.0, dtype=torch.float64, device='cuda')
    P, W, D, Gp = t.data_ptr(), what.data_ptr(), dwhat.data_ptr(), gram.data_ptr()

    def args(dwhat=D, ntan=3, nbytes=n.value, amp=None, clock=None, ids=None):
        return (W, dwhat, ntan, mean.data_ptr(), None, 0, P, nbytes, 2, 64, 64, TWO_PI, TWO_PI, 0.01, 1e-3, 0.1, None, amp, 0, clock, ids, 1, None)
    call = L.nns_spec_ns_step_tangents_f32
    assert call(*args(dwhat=None)) == INVALID and b'dwhat' in L.nns_last_error()
    assert call(*args(ntan=0)) == INVALID and b'ntan' in L.nns_last_error()
    assert call(*args(ntan=33)) == INVALID and b'ntan' in L.nns_last_error()
    assert call(*args(nbytes=n.value - 1)) == WORKSPACE and b'nns_spec_ns_tangents_workspace' in L.nns_last_error()
    assert call(*args(amp=P)) == INVALID
    assert call(*args(amp=P, clock=P)) == INVALID
    assert L.nns_spec_ns_tangent_gram_f64(None, 3, Gp, 2, 64, 64, TWO_PI, TWO_PI, None) == INVALID
    assert L.nns_spec_ns_tangent_gram_f64(D, 0, Gp, 2, 64, 64, TWO_PI, TWO_PI, None) == INVALID
    assert L.nns_spec_ns_tangent_gram_f64(D, 33, Gp, 2, 64, 64, TWO_PI, TWO_PI, None) == INVALID
    assert L.nns_spec_ns_tangent_combine_f32(D, 3, None, 2, 64, 64, None) == INVALID
    assert L.nns_spec_ns_tangent_combine_f32(D, 33, Gp, 2, 64, 64, None) == INVALID
    torch.cuda.synchronize()
    assert bool((what == 3.0).all()) and bool((dwhat == 5.0).all()) and bool((gram == 7.0).all())      # nothing was launched


# ---------------------------------------------------------------------------------------------------- 6. the Gram matrix
def test_gram_against_numpy_symmetric_and_repeatable(gpu_device):
    s, state, dwhat = setup(FORCED, LC.K_ORTHO)
    G = s.tangent_gram(dwhat)
    again = s.tangent_gram(dwhat)
    assert G.dtype == torch.float64 and tuple(G.shape) == (TC.CASES[0][2], LC.K_ORTHO, LC.K_ORTHO)
    assert torch.equal(G, again) and torch.equal(G, G.transpose(1, 2))
    ref = oracle_of(s).gram(expand(s, dwhat))
    err = float(np.abs(host(G) - ref).max() / np.abs(ref).max())
    energy = np.stack([host(s.diagnostics(s._at_rest(dwhat[k])).energy) for k in range(LC.K_ORTHO)], axis=-1)
    diag = np.diagonal(host(G), axis1=1, axis2=2)
    print('MEASURED gram %.2e' % err)
    assert err <= LC.BOUND['gram'], err
    assert np.array_equal(diag, energy)            # the same walk and the same products as ps_diag_kernel: the same bits (LC's note)


# ---------------------------------------------------------------------------------------------------- 7. orthonormalisation
@pytest.mark.parametrize('near', [False, True], ids=['random', 'near'])
def test_orthonormalize_tangents(gpu_device, near):
    c = TC.CASES[0]
    K = LC.K_ORTHO
    s, state, dwhat = setup(FORCED, K, fields=LC.near_fields(c, K) if near else None)
    L = oracle_of(s)
    D0 = expand(s, dwhat)
    logs = s.orthonormalize_tangents(dwhat)
    assert logs.dtype == torch.float64 and tuple(logs.shape) == (c[2], K)
    G = host(s.tangent_gram(dwhat))
    ortho = float(np.abs(G - np.eye(K)).max())
    lerr = float(np.abs(host(logs) - L.qr(D0)[1]).max())
    print('MEASURED ortho_%s %.2e logs_%s %.2e' % ('near' if near else 'random', ortho, 'near' if near else 'random', lerr))
    if not near:
        # the span is kept: the projection of each input on the output basis reproduces it
        Q = expand(s, dwhat)
        W = L.weight()
        dot = lambda a, b: np.einsum('...ij,...ij,ij->...', a.conj(), b, W).real[..., None, None]
        worst = 0.0
        for k in range(K):
            r = D0[k] - sum(dot(Q[l], D0[k]) * Q[l] for l in range(K))
            worst = max(worst, float(np.sqrt(dot(r, r) / dot(D0[k], D0[k])).max()))
        print('MEASURED span %.2e' % worst)
        assert worst <= LC.BOUND['span'], worst
    assert ortho <= LC.BOUND['ortho_near' if near else 'ortho_random'], ortho
    assert lerr <= LC.BOUND['logs'], lerr


def test_a_dependent_pair_gives_nan_in_its_grid_only(gpu_device):
    s, state, dwhat = setup(FORCED, 2)
    dwhat[1, 1] = dwhat[0, 1]
    logs = host(s.orthonormalize_tangents(dwhat))
    assert np.isnan(logs[1]).any() and np.isfinite(logs[0]).all() and np.isfinite(logs[2]).all()
    G = host(s.tangent_gram(dwhat))
    assert np.abs(G[[0, 2]] - np.eye(2)).max() <= LC.BOUND['ortho_random']


# ---------------------------------------------------------------------------------------------------- 8. finite-time exponents against the oracle
@pytest.mark.parametrize('run', LC.SPECTRUM_RUNS, ids=TC.run_id)
def test_finite_time_exponents_against_the_oracle(gpu_device, run):
    s, state, dwhat = setup(run, LC.K_SPECTRUM)
    same = state.clone()
    lam = s.lyapunov_spectrum(state, dwhat, LC.NSTEPS, LC.EVERY)
    assert lam.dtype == torch.float64 and tuple(lam.shape) == (run[1][2], LC.K_SPECTRUM) and state.steps == LC.NSTEPS
    s.step(same, LC.NSTEPS)
    assert torch.equal(state.what, same.what)
    err = float(np.abs(host(lam) - LC.oracle_spectrum(run)).max() * LC.NSTEPS * s.dt)
    ortho = float(np.abs(host(s.tangent_gram(dwhat)) - np.eye(LC.K_SPECTRUM)).max())
    print('MEASURED spectrum %s %.2e (exponents of grid 0: %s); left orthonormal to %.2e' % (run[0], err, host(lam)[0], ortho))
    assert err <= LC.BOUND['spectrum'], err
    assert ortho <= LC.BOUND['ortho_random'], ortho


# ---------------------------------------------------------------------------------------------------- 9. the base at rest
@pytest.mark.parametrize('beta', [0.0, LIN.WAVE_BETA], ids=['drag', 'beta'])
def test_exponents_on_a_base_at_rest(gpu_device, beta):
    """w = 0 with a mean flow: the tangent is advection by the mean flow and the linear operator, so a single mode only decays at
    Re(lambda) = -(nu |k|^2 + drag) (beta turns it, the mean flow translates it), in the order of the vectors: nothing is sorted.  The
    sum of the exponents of A + B and A - B is Re(lambda_A) + Re(lambda_B) at any finite time: the rate of the volume."""
    from nns.periodic import PeriodicSolver
    R = LC.REST
    s = PeriodicSolver(R['nx'], R['ny'], R['dt'], 1.0, R['nu'], drag=R['drag'], **(dict(beta=beta) if beta else {}))
    T = R['nsteps'] * R['dt']
    rest = lambda: s.init_vorticity(torch.zeros((1, R['nx'], R['ny']), device='cuda'), mean=R['mean'])
    state, dwhat = rest(), s.init_tangents(dev(LC.rest_fields()))
    lam = host(s.lyapunov_spectrum(state, dwhat, R['nsteps'], R['every']))[0]
    assert float(state.what.abs().max()) == 0.0
    err = float(np.abs(lam - LC.rest_rates(R['modes'])).max() * T)
    state, dwhat = rest(), s.init_tangents(dev(LC.rest_fields(pair=True)))
    lam2 = host(s.lyapunov_spectrum(state, dwhat, R['nsteps'], R['every']))[0]
    perr = float(abs(lam2.sum() - LC.rest_rates(R['pair']).sum()) * T)
    key = 'beta' if beta else 'drag'
    print('MEASURED rest %s %.2e rest_pair %s %.2e (exponents %s, pair %s)' % (key, err, key, perr, lam, lam2))
    assert err <= LC.BOUND['rest'], err
    assert perr <= LC.BOUND['rest_pair'], perr


# ---------------------------------------------------------------------------------------------------- 10. K = 1 against the single exponent
def test_one_tangent_against_lyapunov_exponent(gpu_device):
    s, state, dwhat = setup(FORCED, 1)
    st1, d1 = state.clone(), dwhat[0].clone()
    lam = host(s.lyapunov_spectrum(state, dwhat, LC.NSTEPS, LC.EVERY))[:, 0]
    ref = host(s.lyapunov_exponent(st1, d1, LC.NSTEPS, LC.EVERY))
    err = float(np.abs(lam - ref).max() * LC.NSTEPS * s.dt)
    print('MEASURED single %.2e (%s against %s)' % (err, lam, ref))
    assert err <= LC.BOUND['single'], err


# ---------------------------------------------------------------------------------------------------- 11. refusals in Python
def test_python_refusals(gpu_device):
    from nns.periodic import PeriodicSolver
    c = TC.CASES[0]
    d = TC.inputs(c)
    s = PeriodicSolver(c[0], c[1], d['dt'], TC.RHO, TC.NU, drag=TC.DRAG, kappa=1e-3)
    state = s.init(dev(d['u0']), dev(d['v0']), dev(d['r']))
    dwhat = s.init_tangents(dev(LC.tangent_fields(c, 2)))
    for call in (lambda: s.step_tangents(state, dwhat, 1), lambda: s.lyapunov_spectrum(state, dwhat, 2, 1)):
        with pytest.raises(NotImplementedError, match='tangent of the scalar system is not built'):
            call()
    free = s.init(dev(d['u0']), dev(d['v0']))
    s.step_tangents(free, dwhat, 1)                                    # a state without a scalar is stepped
    for bad in (dwhat[:, :1], dwhat[0], dwhat.double(), dwhat.cpu(), dwhat.transpose(0, 1).contiguous().transpose(0, 1),
                torch.zeros((33,) + tuple(dwhat.shape[1:]), device='cuda')):
        for call in (lambda: s.step_tangents(free, bad, 1), lambda: s.lyapunov_spectrum(free, bad, 2, 1)):
            with pytest.raises((ValueError, TypeError)):
                call()
    for bad in (dwhat.double(), dwhat.cpu(), torch.zeros((33,) + tuple(dwhat.shape[1:]), device='cuda')):
        for call in (lambda: s.tangent_gram(bad), lambda: s.orthonormalize_tangents(bad)):
            with pytest.raises((ValueError, TypeError)):
                call()
    with pytest.raises(TypeError):
        s.step_tangents(free, None, 1)
    with pytest.raises(ValueError):
        s.init_tangents(torch.zeros((33, 1, c[0], c[1]), device='cuda'))
