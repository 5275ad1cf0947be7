"""GPU checks of K tangent pairs on one base with a scalar and of their Lyapunov spectrum (csrc/pspec_scalar_tangents.hip:
nns_spec_ns_step_scalar_tangents_f32, ps_row_tans_scalar_kernel, the PsScalar + PsTangents + PsTangentsScalar forms of ps_col_kernel,
ps_tangent_variance_gram_kernel; nns.periodic.PeriodicSolver.init_tangents_scalar / step_tangents_scalar / tangent_gram_scalar /
orthonormalize_tangents_scalar / lyapunov_spectrum_scalar) against step_tangent_scalar bit for bit, the float64 restatement
tests/pspec_scalar_lyapunov_oracle.py and the analytic spectrum on a base at rest (tests/pspec_scalar_lyapunov_cases.py)."""
import numpy as np
import pytest
import torch

import pspec_oracle as O
import pspec_scalar_lyapunov_cases as SC
import pspec_scalar_lyapunov_oracle as SLY
import pspec_scalar_tangent_cases as TC

pytestmark = pytest.mark.gpu

C0 = TC.CASES[0]
PASSIVE, BUOYANT, LINEAR, STOCH = SC.SPECTRUM_RUNS
K3 = SC.K_BITWISE


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def setup(run, K, grids=None, fields=None, buoyancy=None):
    """(s, state, dwhat, dthat) of a run on the device: the solver with the case's per-grid force, the state of (u0, v0, theta0) and the K
    tangent pairs; grids: a slice of the batch run alone (with its own noise ids); fields: other pairs than SC.tangent_fields; buoyancy: a
    value that takes the kind's place."""
    kind, c = run
    d = TC.inputs(c)
    sel = slice(None) if grids is None else grids
    s = TC.solver(kind, c, d['dt'], buoyancy=buoyancy)
    s.set_forcing(dev(d['fx'][sel]), dev(d['fy'][sel]))
    state = s.init(dev(d['u0'][sel]), dev(d['v0'][sel]), dev(d['theta0'][sel]))
    if s.stoch_amp is not None:
        state.noise_ids = torch.arange(c[2], dtype=torch.int32, device='cuda')[sel].contiguous()
    dw, dth = SC.tangent_fields(c, K) if fields is None else fields
    dwhat, dthat = s.init_tangents_scalar(dev(dw[:, sel]), dev(dth[:, sel]))
    return s, state, dwhat, dthat


def singles(s, state, dwhat, dthat, nsteps, members=None):
    """What step_tangent_scalar gives for each member alone from a clone of the state: [(k, state_k, dwhat_k, dthat_k)]."""
    out = []
    for k in range(dwhat.shape[0]) if members is None else members:
        st, dk, tk = state.clone(), dwhat[k].clone(), dthat[k].clone()
        s.step_tangent_scalar(st, dk, tk, nsteps)
        out.append((k, st, dk, tk))
    return out


def expand(s, spec):
    """complex128 rfft2-layout spectra [..., nx, nh] of compact float32 spectra [..., my1, nx, 2] (zero beyond the kept y-wavenumbers)."""
    z = host(spec)
    z = np.swapaxes(z[..., 0] + 1j * z[..., 1], -1, -2)
    out = np.zeros(z.shape[:-1] + (s.ny // 2 + 1,), dtype=np.complex128)
    out[..., :s.my1] = z
    return out


def oracle_of(weight=1.0, kind='buoyant'):
    return SLY.ScalarLyapunov(TC.scheme(kind, C0, TC.inputs(C0)['dt']), weight)


# ---------------------------------------------------------------------------------------------------- 1. bitwise against step and step_tangent_scalar
@pytest.mark.parametrize('run', TC.RUNS, ids=TC.run_id)
def test_base_and_every_member_are_bitwise_step_and_step_tangent_scalar(gpu_device, run):
    s, state, dwhat, dthat = setup(run, K3)
    n = SC.NSTEPS_BITWISE
    same = state.clone()
    s.step(same, n)
    ref = singles(s, state, dwhat, dthat, n)
    bw, bt = dwhat.clone(), dthat.clone()
    out = s.step_tangents_scalar(state, dwhat, dthat, n)
    assert out[0] is dwhat and out[1] is dthat and not torch.equal(dwhat, bw) and not torch.equal(dthat, bt)
    assert torch.equal(state.what, same.what) and torch.equal(state.that, same.that) and state.steps == same.steps == n
    if s.stoch_amp is not None:
        assert torch.equal(state.clock, same.clock) and int(state.clock) == n
    for k, st, dk, tk in ref:
        assert torch.equal(st.what, state.what) and torch.equal(st.that, state.that)
        assert torch.equal(dwhat[k], dk), 'dwhat of member %d' % k
        assert torch.equal(dthat[k], tk), 'dthat of member %d' % k
        assert torch.equal(dthat[k, :, 0, 0], bt[k, :, 0, 0])           # the mean of dtheta is carried bit for bit
        assert float(bt[k, :, 0, 0, 0].abs().min()) > 0


# ---------------------------------------------------------------------------------------------------- 2. - 5. K and neighbours do not matter
def test_a_member_does_not_depend_on_K(gpu_device):
    s, state, dwhat, dthat = setup(BUOYANT, 5)
    outs = []
    for K in (1, 2, 5):
        st, dw, dt = state.clone(), dwhat[:K].clone(), dthat[:K].clone()
        s.step_tangents_scalar(st, dw, dt, 2)
        outs.append((st, dw, dt))
    for st, dw, dt in outs[:2]:
        assert torch.equal(dw[0], outs[2][1][0]) and torch.equal(dt[0], outs[2][2][0])
        assert torch.equal(st.what, outs[2][0].what) and torch.equal(st.that, outs[2][0].that)
    assert torch.equal(outs[1][1][1], outs[2][1][1]) and torch.equal(outs[1][2][1], outs[2][2][1])


def test_K_32_first_and_last_member(gpu_device):
    c = (64, 64, 1) + C0[3:]
    s, state, dwhat, dthat = setup(('buoyant', c), 32)
    ref = singles(s, state, dwhat, dthat, 1, members=(0, 31))
    s.step_tangents_scalar(state, dwhat, dthat, 1)
    for k, st, dk, tk in ref:
        assert torch.equal(dwhat[k], dk) and torch.equal(dthat[k], tk) and torch.equal(st.what, state.what) and torch.equal(st.that, state.that)
    assert float(dwhat[31].abs().max()) > 0 and float(dthat[31].abs().max()) > 0


@pytest.mark.parametrize('run', [BUOYANT, STOCH], ids=TC.run_id)
def test_a_batch_is_its_grids_and_one_call_is_chained_calls(gpu_device, run):
    s, state, dwhat, dthat = setup(run, K3)
    s.step_tangents_scalar(state, dwhat, dthat, 3)
    for b in range(run[1][2]):
        s1, st1, d1, t1 = setup(run, K3, grids=slice(b, b + 1))
        s1.step_tangents_scalar(st1, d1, t1, 3)
        assert torch.equal(d1[:, 0], dwhat[:, b]) and torch.equal(t1[:, 0], dthat[:, b])
        assert torch.equal(st1.what[0], state.what[b]) and torch.equal(st1.that[0], state.that[b])
    s, st, dw, dt = setup(run, K3)
    for _ in range(3):
        s.step_tangents_scalar(st, dw, dt, 1)
    assert torch.equal(dw, dwhat) and torch.equal(dt, dthat) and torch.equal(st.what, state.what) and torch.equal(st.that, state.that) and st.steps == 3


def test_grid_stride(gpu_device):
    c = SC.GRID_STRIDE
    nx, ny, B = c[:3]
    u0, v0, dt = TC.C.full_band_input(nx, ny, 4, c[3], c[4], c[5])
    idx = np.array([0, 1] + [2, 3] * ((B - 2) // 2))                   # the first two grids and the last two differ
    th0 = O.band_ic(4, nx, ny, 3, c[3], c[4], 1.0)[0]
    dw = np.stack([O.band_ic(4, nx, ny, 5 + 100 * k, c[3], c[4], 1.0)[0] for k in range(2)])
    dth = np.stack([O.band_ic(4, nx, ny, 6 + 100 * k, c[3], c[4], 1.0)[0] + 0.3 for k in range(2)])
    s = TC.solver('buoyant', c, dt)
    outs = []
    for sel in (idx, idx[:2], idx[-2:]):
        state = s.init(dev(u0[sel]), dev(v0[sel]), dev(th0[sel]))
        dwhat, dthat = s.init_tangents_scalar(dev(dw[:, sel]), dev(dth[:, sel]))
        s.step_tangents_scalar(state, dwhat, dthat, 1)
        outs.append((state.what, state.that, dwhat, dthat))
    full, first, last = outs
    for a, b01, b23 in zip(full[:2], first[:2], last[:2]):
        assert torch.equal(a[:2], b01) and torch.equal(a[-2:], b23)
    for a, b01, b23 in zip(full[2:], first[2:], last[2:]):
        assert torch.equal(a[:, :2], b01) and torch.equal(a[:, -2:], b23)
    assert float(full[2][1].abs().max()) > 0 and float(full[3][1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 6. eager equals graph replay
@pytest.mark.parametrize('run', [BUOYANT, STOCH], ids=TC.run_id)
def test_eager_equals_graph_replay(gpu_device, run):
    s, eager, dwe, dte = setup(run, 2)
    s.step_tangents_scalar(eager, dwe, dte, 1)                          # grows the workspace, loads the code objects
    st, dw, dt = eager.clone(), dwe.clone(), dte.clone()
    s.step_tangents_scalar(eager, dwe, dte, 2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.step_tangents_scalar(st, dw, dt, 1)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dw, dwe) and torch.equal(dt, dte) and torch.equal(st.what, eager.what) and torch.equal(st.that, eager.that)
    if s.stoch_amp is not None:
        assert int(st.clock) == int(eager.clock) == 3


# ---------------------------------------------------------------------------------------------------- 7. b = 0: dwhat is step_tangents' on the flow alone
def test_without_buoyancy_dwhat_is_bitwise_step_tangents(gpu_device):
    s, state, dwhat, dthat = setup(PASSIVE, K3)
    free = s.init(*(dev(TC.inputs(C0)[k]) for k in ('u0', 'v0')))
    assert free.that is None and torch.equal(free.what, state.what)
    flow = dwhat.clone()
    s.step_tangents(free, flow, 3)
    s.step_tangents_scalar(state, dwhat, dthat, 3)
    assert torch.equal(dwhat, flow) and torch.equal(state.what, free.what)


# ---------------------------------------------------------------------------------------------------- 8. the workspace
def test_the_call_stays_inside_its_workspace(gpu_device):
    from nns import ops
    s, ref_state, ref_w, ref_t = setup(BUOYANT, K3, grids=slice(0, 1))
    s.step_tangents_scalar(ref_state, ref_w, ref_t, 2)
    s, state, dwhat, dthat = setup(BUOYANT, K3, grids=slice(0, 1))
    need = ops.spec_ns_scalar_tangents_workspace(1, K3, s.nx, s.ny)
    assert need == max((10 + 10 * 3) * 64 * 22 * 8, ops.spec_ns_workspace(1, 64, 64)) and need >= ops.spec_ns_workspace(1, 64, 64)
    assert ops.spec_ns_scalar_tangents_workspace(1, 1, 64, 64) == ops.spec_ns_scalar_tangent_workspace(1, 64, 64)
    buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
    state.work = buf[:need]
    s.step_tangents_scalar(state, dwhat, dthat, 2)
    assert state.work.data_ptr() == buf.data_ptr()
    assert bool((buf[need:] == 0xA5).all())
    assert torch.equal(dwhat, ref_w) and torch.equal(dthat, ref_t) and torch.equal(state.what, ref_state.what) and torch.equal(state.that, ref_state.that)


# ---------------------------------------------------------------------------------------------------- 9. the variance Gram matrix
def test_variance_gram_against_numpy_symmetric_repeatable_and_blind_to_the_mean(gpu_device):
    from nns import ops
    K = SC.K_ORTHO
    s, state, dwhat, dthat = setup(BUOYANT, K)
    G = ops.spec_ns_tangent_variance_gram(dthat, s.ny)
    again = ops.spec_ns_tangent_variance_gram(dthat, s.ny)
    assert G.dtype == torch.float64 and tuple(G.shape) == (C0[2], K, K)
    assert torch.equal(G, again) and torch.equal(G, G.transpose(1, 2))
    L = oracle_of()
    zero = np.zeros_like(expand(s, dwhat))
    ref = L.gram(zero, expand(s, dthat))
    err = float(np.abs(host(G) - ref).max() / np.abs(ref).max())
    var = np.stack([host(ops.spec_ns_scalar_diag(dwhat[k], dthat[k], s.ny, s.Lx, s.Ly, s.kappa)[:, 0]) for k in range(K)], axis=-1)
    assert np.array_equal(np.diagonal(host(G), axis1=1, axis2=2), var)  # ps_scalar_diag_kernel's walk and term: the same bits
    moved = dthat.clone()
    moved[:, :, 0, 0, 0] += 7.0
    moved[:, :, 0, 0, 1] = 3.0
    assert torch.equal(ops.spec_ns_tangent_variance_gram(moved, s.ny), G)
    for weight in (1.0, SC.WEIGHT):                                     # the pair's Gram matrix is the sum of the two
        Gp = s.tangent_gram_scalar(dwhat, dthat, weight)
        pref = oracle_of(weight).gram(expand(s, dwhat), expand(s, dthat))
        err = max(err, float(np.abs(host(Gp) - pref).max() / np.abs(pref).max()))
        assert torch.equal(Gp, s.tangent_gram(dwhat) + weight * G) and torch.equal(Gp, Gp.transpose(1, 2))
    print('MEASURED gram %.2e' % err)
    assert err <= SC.BOUND['gram'], err


# ---------------------------------------------------------------------------------------------------- 10. orthonormalisation
@pytest.mark.parametrize('weight', [1.0, SC.WEIGHT])
@pytest.mark.parametrize('near', [False, True], ids=['random', 'near'])
def test_orthonormalize_tangents_scalar(gpu_device, near, weight):
    K = SC.K_ORTHO
    s, state, dwhat, dthat = setup(BUOYANT, K, fields=SC.near_fields(C0, K) if near else None)
    L = oracle_of(weight)
    Dw, Dt = expand(s, dwhat), expand(s, dthat)
    logs = s.orthonormalize_tangents_scalar(dwhat, dthat, weight)
    assert logs.dtype == torch.float64 and tuple(logs.shape) == (C0[2], K)
    G = host(s.tangent_gram_scalar(dwhat, dthat, weight))
    ortho = float(np.abs(G - np.eye(K)).max())
    lerr = float(np.abs(host(logs) - L.qr(Dw, Dt)[2]).max())
    tag = 'near' if near else 'random'
    print('MEASURED ortho_%s %.2e logs_%s %.2e (weight %g)' % (tag, ortho, tag, lerr, weight))
    assert ortho <= SC.BOUND['ortho_near' if near else 'ortho_random'], ortho
    assert lerr <= SC.BOUND['logs'], lerr


def test_a_dependent_pair_gives_nan_in_its_grid_only(gpu_device):
    s, state, dwhat, dthat = setup(BUOYANT, 2)
    dwhat[1, 1], dthat[1, 1] = dwhat[0, 1], dthat[0, 1]
    logs = host(s.orthonormalize_tangents_scalar(dwhat, dthat))
    assert np.isnan(logs[1]).any() and np.isfinite(logs[0]).all() and np.isfinite(logs[2]).all()
    G = host(s.tangent_gram_scalar(dwhat, dthat))
    assert np.abs(G[[0, 2]] - np.eye(2)).max() <= SC.BOUND['ortho_random']


# ---------------------------------------------------------------------------------------------------- 11. finite-time exponents against the oracle
@pytest.mark.parametrize('run,weight', [(r, 1.0) for r in SC.SPECTRUM_RUNS] + [(BUOYANT, SC.WEIGHT)],
                         ids=lambda v: TC.run_id(v) if isinstance(v, tuple) else 'w%g' % v)
def test_finite_time_exponents_against_the_oracle(gpu_device, run, weight):
    K = SC.K_SPECTRUM
    s, state, dwhat, dthat = setup(run, K)
    same = state.clone()
    lam = s.lyapunov_spectrum_scalar(state, dwhat, dthat, SC.NSTEPS, SC.EVERY, scalar_weight=weight)
    assert lam.dtype == torch.float64 and tuple(lam.shape) == (run[1][2], K) and state.steps == SC.NSTEPS
    s.step(same, SC.NSTEPS)
    assert torch.equal(state.what, same.what) and torch.equal(state.that, same.that)
    err = float(np.abs(host(lam) - SC.oracle_spectrum(run, None, weight)).max() * SC.NSTEPS * s.dt)
    ortho = float(np.abs(host(s.tangent_gram_scalar(dwhat, dthat, weight)) - np.eye(K)).max())
    print('MEASURED spectrum %s weight %g %.2e (exponents of grid 0: %s); left orthonormal to ortho_random %.2e' % (run[0], weight, err, host(lam)[0], ortho))
    assert err <= SC.BOUND['spectrum'], err
    assert ortho <= SC.BOUND['ortho_random'], ortho


# ---------------------------------------------------------------------------------------------------- 12. the base at rest
@pytest.mark.parametrize('weight', [1.0, SC.WEIGHT])
def test_the_spectrum_on_the_base_at_rest(gpu_device, weight):
    """Base at rest with the mean flow U, b . G < 0: the K = 4 vectors of SC.rest_fields give (lambda_+, lambda_+, lambda_-, lambda_-) at any
    finite time and for any scalar_weight (that function's note); the restatement reproduces it to 4.66e-10."""
    from nns.periodic import PeriodicSolver
    p = SC.EIGEN
    n = p['nsteps']
    s = PeriodicSolver(p['nx'], p['ny'], p['dt'], 1.0, p['nu'], drag=p['drag'], kappa=p['kappa'], scalar_gradient=p['G'], buoyancy=p['b'])
    zero = torch.zeros((1, p['nx'], p['ny']), device='cuda')
    state = s.init_vorticity(zero, mean=p['U'])
    state = s._with_scalar('test', state, zero)
    dwhat, dthat = s.init_tangents_scalar(*(dev(f) for f in SC.rest_fields()))
    lam = host(s.lyapunov_spectrum_scalar(state, dwhat, dthat, n, SC.REST_EVERY, scalar_weight=weight))[0]
    assert float(state.what.abs().max()) == 0.0 and state.steps == n
    lp, lm = SC.rest_rates()[:2]
    err = float(np.abs(lam - np.array([lp, lp, lm, lm])).max() * n * p['dt'])
    print('MEASURED rest weight %g %.2e (exponents %s against %.9f, %.9f)' % (weight, err, lam, lp, lm))
    assert err <= SC.BOUND['rest'], err


# ---------------------------------------------------------------------------------------------------- 13. K = 1 against the single exponent
@pytest.mark.parametrize('weight', [1.0, SC.WEIGHT])
def test_one_pair_against_lyapunov_exponent_scalar(gpu_device, weight):
    s, state, dwhat, dthat = setup(BUOYANT, 1)
    st1, d1, t1 = state.clone(), dwhat[0].clone(), dthat[0].clone()
    lam = host(s.lyapunov_spectrum_scalar(state, dwhat, dthat, SC.NSTEPS, SC.EVERY, scalar_weight=weight))[:, 0]
    ref = host(s.lyapunov_exponent_scalar(st1, d1, t1, SC.NSTEPS, SC.EVERY, scalar_weight=weight))
    err = float(np.abs(lam - ref).max() * SC.NSTEPS * s.dt)
    print('MEASURED single weight %g %.2e (%s against %s)' % (weight, err, lam, ref))
    assert err <= SC.BOUND['single'], err


# ---------------------------------------------------------------------------------------------------- 14. refusals in Python
def test_python_refusals(gpu_device):
    from nns.periodic import PeriodicSolver
    c = C0
    d = TC.inputs(c)
    s, state, dwhat, dthat = setup(BUOYANT, 2)
    free = s.init(dev(d['u0']), dev(d['v0']))
    every = lambda st, a, b: (lambda: s.step_tangents_scalar(st, a, b, 1), lambda: s.lyapunov_spectrum_scalar(st, a, b, 2, 1))
    for call in every(free, dwhat, dthat):                              # a state without a scalar
        with pytest.raises(ValueError, match='step_tangents|lyapunov_spectrum'):
            call()
    bare = PeriodicSolver(c[0], c[1], d['dt'], TC.RHO, TC.NU, drag=TC.DRAG)      # a solver without kappa
    for call in (lambda: bare.step_tangents_scalar(bare.init(dev(d['u0']), dev(d['v0'])), dwhat, dthat, 1),
                 lambda: bare.tangent_gram_scalar(dwhat, dthat), lambda: bare.orthonormalize_tangents_scalar(dwhat, dthat),
                 lambda: bare.init_tangents_scalar(*(dev(f) for f in SC.tangent_fields(c, 2)))):
        with pytest.raises(ValueError, match='kappa'):
            call()
    wide = torch.zeros((33,) + tuple(dwhat.shape[1:]), device='cuda')
    bads = [(bad, dthat) for bad in (dwhat[:, :1], dwhat[0], dwhat.double(), dwhat.cpu(), dwhat.transpose(0, 1).contiguous().transpose(0, 1),
                                     dwhat[:1].contiguous(), wide)]         # wrong batch, rank, dtype, device, strides, K of one half, K = 33
    for a, b in bads + [(b, a) for a, b in bads] + [(wide, wide)]:
        for call in every(state, a, b) + (lambda: s.tangent_gram_scalar(a, b), lambda: s.orthonormalize_tangents_scalar(a, b)):
            with pytest.raises((ValueError, TypeError)):
                call()
    for call in every(state, None, dthat) + every(state, dwhat, None):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        s.init_tangents_scalar(torch.zeros((33, 1, c[0], c[1]), device='cuda'), torch.zeros((33, 1, c[0], c[1]), device='cuda'))
    with pytest.raises(ValueError):
        s.init_tangents_scalar(*(dev(f) for f in (SC.tangent_fields(c, 2)[0], SC.tangent_fields(c, 3)[1])))
    for w in (0.0, -1.0, float('nan')):
        for call in (lambda: s.tangent_gram_scalar(dwhat, dthat, w), lambda: s.orthonormalize_tangents_scalar(dwhat, dthat, w),
                     lambda: s.lyapunov_spectrum_scalar(state, dwhat, dthat, 2, 1, scalar_weight=w)):
            with pytest.raises(ValueError, match='scalar_weight'):
                call()
    with pytest.raises(TypeError):
        s.tangent_gram_scalar(dwhat, dthat, '1')
    before = (state.what.clone(), dwhat.clone(), dthat.clone())
    for call in (lambda: s.step_tangents(state, dwhat, 1), lambda: s.lyapunov_spectrum(state, dwhat, 2, 1)):      # the old entry points still refuse
        with pytest.raises(NotImplementedError, match='tangent of the scalar system is not built'):
            call()
    assert torch.equal(state.what, before[0]) and torch.equal(dwhat, before[1]) and torch.equal(dthat, before[2]) and state.steps == 0
    s.step_tangents_scalar(state, dwhat, dthat, 1)                      # and the pair is stepped
    assert state.steps == 1
