"""GPU checks of the general linear operator of the pseudo-spectral periodic solver -- hyperviscosity, hypofriction and the beta effect in the
Lawson factor (csrc/pspec_kernels.hip: nns_spec_ns_step_linear_f32, nns_spec_ns_linear_spectrum_f32, through nns.periodic.PeriodicSolver) --
against the restatement tests/pspec_linear_oracle.py: trajectories at every shape where the table's indexing can go wrong, the grid-stride
loop, the analytic Rossby wave, a stiff step, the call patterns that must give the same bits, the linear rates per shell, the inactive path
that must stay what it is, and the refusals.  The figures measured on the MI355X are in tests/pspec_linear_cases.py: MEASURED."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pspec_buoyant_cases as BC
import pspec_cases as C
import pspec_forced_cases as FC
import pspec_linear_cases as LC
import pspec_linear_oracle as LO
import pspec_scalar_cases as SC
import pspec_spectrum_cases as PC
import pspec_spectrum_oracle as PO
import pspec_stochastic_cases as XC
from conftest import rel_l2

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device='cuda')          # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy().astype(np.float64)


def state_c(t):
    w = host(t)
    return w[..., 0] + 1j * w[..., 1]


# ---------------------------------------------------------------------------------------------------- 1. trajectories against the float64 oracle
TRAJ = [('flow', c) for c in LC.CASES] + [('scalar', LC.SCALAR_CASE), ('buoyant', LC.BUOYANT_CASE), ('stochastic', LC.CASES[0])]
TRAJ_IDS = LC.CASE_IDS + ['64x64-scalar', '64x64-buoyant', '64x64-stochastic']


@pytest.mark.parametrize('kind, case', TRAJ, ids=TRAJ_IDS)
def test_trajectory_against_the_oracle(gpu_device, kind, case):
    # NSTEPS steps of the full-band inputs with every term of pspec_linear_cases acting, within the bounds of the deterministic step
    # (C.BOUND_W, C.BOUND_UV, C.BOUND_P; BC.BOUND_P for the buoyant pressure).  Each wrong scheme is >= 10 x those bounds away
    # (tests/test_oracle_pspec_linear.py).  Measured figures: LC.MEASURED.
    nx, ny, B, Lx, Ly, _ = case
    S, ins, w, t, mean, extra = LC.reference(kind, case)
    stoch = None if extra is None else (extra[0],) + tuple(XC.traj_ring(nx, ny, Lx, Ly))
    s = LC.solver(case, S.dt, 'flow' if kind == 'stochastic' else kind, stochastic=stoch)
    assert s._linear() and SC.rel_l2c(s.linear_operator(), S.compact(S.linear_operator())) <= 1e-14
    if extra is not None:
        assert np.array_equal(s.stoch_amp, extra[1])
    st = s.init(*[dev(a) for a in ins])
    s.step(st, LC.NSTEPS)
    ew = SC.rel_l2c(state_c(st.what), S.compact(w))
    got = [host(f) for f in s.fields(st)]
    ref = S.fields(w, mean, t) if kind == 'buoyant' else S.fields(w, mean)
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    et = 0.0 if t is None else SC.rel_l2c(S.compact(S.fluctuation(S.expand(state_c(st.that)))), S.compact(S.fluctuation(t)))
    print('linear %s %dx%d B=%d dt=%.2e, %d steps: rel-L2 what %.2e, that\' %.2e; u, v, p %s'
          % (kind, nx, ny, B, S.dt, LC.NSTEPS, ew, et, ['%.2e' % e for e in errs]))
    assert ew <= C.BOUND_W and et <= C.BOUND_W, (ew, et)
    assert max(errs[:2]) <= C.BOUND_UV, errs
    assert errs[2] <= (BC.BOUND_P if kind == 'buoyant' else C.BOUND_P), errs
    assert st.steps == LC.NSTEPS and (extra is None or int(st.clock) == LC.NSTEPS)


# ---------------------------------------------------------------------------------------------------- 2. the grid-stride loop
def test_grid_stride_loop_gives_the_bits_of_small_batches(gpu_device):
    # (1024, 64, 400), one step: 8800 columns in 2200 tiles of 4 lines, more than the 2048 workgroups of the launch; the first and the last two
    # grids are bitwise those of the same grids stepped as batches of 2 (the table is shared by the batch, indexed by the line alone)
    nx, ny, B, Lx, Ly, mean = LC.STRIDE_CASE
    u2, v2, dt = C.full_band_input(nx, ny, 4, Lx, Ly, mean)
    idx = torch.arange(B, device='cuda') % 4
    idx[-2:] = torch.tensor([2, 3], device='cuda')
    u, v = dev(u2)[idx], dev(v2)[idx]
    s = LC.solver(LC.STRIDE_CASE, dt)
    big = s.step(s.init(u, v), 1)
    for sl in (slice(0, 2), slice(B - 2, B)):
        small = s.step(s.init(u[sl].clone(), v[sl].clone()), 1)
        assert torch.equal(small.what, big.what[sl])
    assert not torch.equal(big.what[0], big.what[1]) and bool(torch.isfinite(big.what).all())
    assert torch.equal(big.what[4:8], big.what[0:4])


# ---------------------------------------------------------------------------------------------------- 3. the Rossby wave, 200 steps
def test_rossby_wave_with_mean_flow_200_steps(gpu_device):
    # tests/test_oracle_pspec_linear.py::test_rossby_wave_with_mean_flow_200_steps on the GPU: the scheme's own error is 5e-9 of the amplitude,
    # so what is measured is float32.  Bound: LC.WAVE_BOUND, that of the buoyant plane waves.
    from nns.periodic import PeriodicSolver
    nx, ny, Lx, Ly, m, U, dt = LC.WAVE
    n = LC.WAVE_STEPS
    s = PeriodicSolver(nx, ny, dt, C.RHO, LC.WAVE_NU, Lx=Lx, Ly=Ly, drag=LC.WAVE_DRAG, hyperviscosity=LC.WAVE_HYPER, hypofriction=LC.WAVE_HYPO,
                       beta=LC.WAVE_BETA)
    u0, v0 = LO.rossby_wave(nx, ny, 0.0, m, LC.WAVE_BETA, LC.wave_damping(), U, Lx, Ly)[:2]
    st = s.init(dev(u0), dev(v0))
    s.step(st, n)
    ru, rv, rw, A, om = LO.rossby_wave(nx, ny, n * dt, m, LC.WAVE_BETA, LC.wave_damping(), U, Lx, Ly)
    S = LO.LinearScheme(nx, ny, dt, C.RHO, LC.WAVE_NU, Lx, Ly)
    wf = S.irfft2(S.expand(state_c(st.what)))[0]
    u, v, p = [host(f)[0] for f in s.fields(st)]
    ew = np.abs(wf - rw).max() / A
    eu = max(np.abs(u - ru).max(), np.abs(v - rv).max()) / A
    print('Rossby wave %dx%d m %s on U %s, %d steps: omega t = %.3f rad, amplitude %.4f; max error / amplitude: w %.2e, u and v %.2e'
          % (nx, ny, m, U, n, om * n * dt, A, ew, eu))
    assert abs(om * n * dt) > 3 and A >= 0.4
    assert max(ew, eu) <= LC.WAVE_BOUND, (ew, eu)
    assert np.abs(p).max() <= 1e-5                                                  # a plane wave has no pressure


# ---------------------------------------------------------------------------------------------------- 4. stiffness
def test_a_stiff_step_stays_finite_and_matches_the_oracle(gpu_device):
    # nu_h K^2p dt = 50 in one step: the corner's factor is exp(-50); an explicit RK4 is unstable beyond 2.8 and would blow up
    case = LC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    u0, v0, dt = C.full_band_input(*case)
    pr = LC.params(nx, ny, Lx, Ly, dt, hyper_per_step=LC.STIFF_PER_STEP)
    assert abs(pr['hyper'][0] * LC.corner(nx, ny, Lx, Ly) ** 8 * dt - 50) < 1e-9
    S = LC.scheme(nx, ny, dt, Lx, Ly, hyper=pr['hyper'])
    w0, mean = S.init(u0, v0)
    w = S.step(w0, mean, 1)
    s = LC.solver(case, dt, hyperviscosity=pr['hyper'])
    st = s.step(s.init(dev(u0), dev(v0)), 1)
    assert bool(torch.isfinite(st.what).all())
    ew = SC.rel_l2c(state_c(st.what), S.compact(w))
    errs = [rel_l2(host(g), r) for g, r in zip(s.fields(st), S.fields(w, mean))]
    print('stiff step 64x64 (nu_h K^8 dt = 50): rel-L2 what %.2e; u, v, p %s; enstrophy left %.3f' % (ew, ['%.2e' % e for e in errs],
                                                                                                 np.mean(S.diag(w)[1] / S.diag(w0)[1])))
    assert ew <= C.BOUND_W and max(errs[:2]) <= C.BOUND_UV and errs[2] <= C.BOUND_P, (ew, errs)


# ---------------------------------------------------------------------------------------------------- 5. call patterns, graph replay, Hermitian line
def test_eager_loop_one_call_and_graph_replay_are_bitwise_equal(gpu_device):
    case = LC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    u0, v0, dt = C.full_band_input(*case)
    s = LC.solver(case, dt)
    eager = s.simulate(dev(u0), dev(v0), 12, save_every=1, use_graph=False)
    assert s.last_simulate_used_graph is False
    graphed = s.simulate(dev(u0), dev(v0), 12, save_every=1, use_graph=True)
    assert s.last_simulate_used_graph is True
    for a, b in zip(eager, graphed):
        assert a.shape == (13, B, nx, ny) and torch.equal(a, b)
    once, many = s.init(dev(u0), dev(v0)), s.init(dev(u0), dev(v0))
    s.step(once, 12)
    for _ in range(12):
        s.step(many, 1)
    assert torch.equal(once.what, many.what) and once.steps == many.steps == 12
    for a, b in zip(s.fields(once), eager):
        assert torch.equal(a, b[12])
    # the j = 0 line stores +m_x and -m_x, each with its own factor from the table: conjugate to rounding (bound: 100 float32 ulp of the
    # line's largest element, as for the stochastic step)
    line = state_c(once.what[:, 0])
    defect = np.abs(line[:, 1:nx // 2] - np.conj(line[:, :nx // 2:-1])).max() / np.abs(line).max()
    print('j = 0 line after 12 linear steps: Hermitian defect %.2e of the largest element' % defect)
    assert defect <= 100 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- 6. the linear rates per shell
def test_linear_spectrum_against_the_oracle_and_the_budget(gpu_device):
    # both sides sum the same float32 spectrum in float64 (PC.BOUND_SPECTRUM, the bound of E and Z in tests/test_gpu_pspec_spectrum.py)
    case = LC.CASES[1]
    nx, ny, B, Lx, Ly, _ = case
    S, ins, w, t, mean, _ = LC.reference('flow', case)
    s = LC.solver(case, S.dt)
    st = s.step(s.init(*[dev(a) for a in ins]), LC.NSTEPS)
    before = st.what.clone()
    lr = s.linear_spectrum(st)
    k, dk = s.shells()
    nS = len(k)
    assert lr._fields == ('k', 'energy', 'enstrophy') and np.array_equal(lr.k, k)
    assert all(x.dtype == torch.float64 and tuple(x.shape) == (B, nS) and x.is_cuda for x in lr[1:]) and torch.equal(st.what, before)
    T = LC.scheme(nx, ny, S.dt, Lx, Ly)
    T.g = T.expand(state_c(s.ghat))
    wg = T.expand(state_c(st.what))
    DE, DZ = T.linear_spectrum(wg)
    errs = []
    for got, r in ((lr.energy, DE), (lr.enstrophy, DZ)):
        got = got.cpu().numpy()
        live = r < 0
        assert (got[~live] == 0).all() and live[:, -1].all() and not live[:, 0].any()
        errs.append(np.abs(got[live] / r[live] - 1).max())
    # the budget is T_E + F + D_E, and its total is power_in + sum D_E up to sum_s T_E, which vanishes to the transfer's float32 rounding
    sp, tr, bud, d = s.spectrum(st), s.transfer(st), s.energy_budget(st), s.diagnostics(st)
    assert torch.equal(bud, tr.energy + sp.injection + lr.energy)
    scale = PO.transfer(T, wg)['A_E'].sum(axis=-1)
    closure = np.abs((bud.sum(-1) - (d.power_in + lr.energy.sum(-1))).cpu().numpy()) / scale
    print('linear_spectrum %dx%d S=%d: D_E %.1e, D_Z %.1e (relative, per shell); total budget against power_in + sum D_E: %.2e of the transfer scale'
          % (nx, ny, nS, errs[0], errs[1], closure.max()))
    assert max(errs) <= PC.BOUND_SPECTRUM, errs
    assert closure.max() <= PC.BOUND_TRANSFER
    # beta does not enter, and an inactive solver gives -2 nu Z - 2 drag E
    nobeta = LC.solver(case, S.dt, beta=0.0).linear_spectrum(st)
    assert torch.equal(nobeta.energy, lr.energy) and torch.equal(nobeta.enstrophy, lr.enstrophy)
    from nns.periodic import PeriodicSolver
    plain = PeriodicSolver(nx, ny, S.dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=LC.DRAG)
    assert not plain._linear()
    pl = plain.linear_spectrum(st)
    ref = (-2 * C.NU * sp.enstrophy - 2 * LC.DRAG * sp.energy).cpu().numpy()
    got = pl.energy.cpu().numpy()
    live = ref < 0
    e = np.abs(got[live] / ref[live] - 1).max()
    print('inactive solver: D_E against -2 nu Z - 2 drag E: %.1e relative' % e)
    assert e <= PC.BOUND_SPECTRUM and (got[~live] == 0).all()
    assert np.array_equal(plain.linear_operator().imag, np.zeros((s.my1, nx)))


# ---------------------------------------------------------------------------------------------------- 7. inactive is identical
@pytest.mark.parametrize('kind', ['forced', 'buoyant', 'stochastic'])
def test_zero_parameters_are_bitwise_the_solver_without_the_arguments(gpu_device, kind):
    from nns.periodic import PeriodicSolver
    case = LC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    u0, v0, dt = C.full_band_input(*case)
    th0 = SC.scalar_input(*case) if kind == 'buoyant' else None
    kw = dict(kappa=SC.KAPPA, scalar_gradient=SC.GRAD, buoyancy=BC.BUOY) if kind == 'buoyant' else {}
    runs = []
    for extra in ({}, dict(hyperviscosity=(0.0, 4), hypofriction=(0.0, 1), beta=0.0), dict(beta=1e-3)):
        s = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=FC.DRAG, **dict(kw, **extra)).kolmogorov_forcing(FC.KF, FC.AMP)
        if kind == 'stochastic':
            s.ring_forcing(1.0, 4, 6, seed=XC.SEED)
        st = s.init(dev(u0), dev(v0), None if th0 is None else dev(th0))
        s.step(st, LC.NSTEPS)
        runs.append((s, st))
    (sa, a), (sb, b), (sc, c) = runs
    assert not sa._linear() and not sb._linear() and sc._linear() and sb._lin is None and not sb._lin_dev
    assert torch.equal(a.what, b.what) and (th0 is None or torch.equal(a.that, b.that))
    assert torch.equal(sa.energy_budget(a), sb.energy_budget(b))
    assert not torch.equal(c.what, a.what)
    # a small beta is a small change: the linear path continues the plain one
    assert SC.rel_l2c(state_c(c.what), state_c(a.what)) < 1e-2


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_argument_errors(gpu_device):
    from nns import ops, _lib
    from nns.periodic import PeriodicSolver
    mk = lambda **kw: PeriodicSolver(64, 64, 0.01, 1.0, 1e-3, **kw)
    for bad in (dict(hyperviscosity=1.0), dict(hyperviscosity=(1.0,)), dict(hyperviscosity=('a', 4)), dict(hyperviscosity=(1.0, 4.0)),
                dict(hyperviscosity=(1.0, True)), dict(hypofriction=(1.0, 1.5)), dict(hypofriction=3), dict(beta='x'), dict(beta=None),
                dict(beta=True), dict(hyperviscosity=(True, 4))):
        with pytest.raises(TypeError):
            mk(**bad)
    for bad in (dict(hyperviscosity=(-1.0, 4)), dict(hyperviscosity=(1.0, 1)), dict(hyperviscosity=(1.0, 9)), dict(hyperviscosity=(math.inf, 4)),
                dict(hypofriction=(-1.0, 1)), dict(hypofriction=(1.0, 0)), dict(hypofriction=(1.0, 5)), dict(hypofriction=(math.nan, 1)),
                dict(beta=math.inf), dict(beta=math.nan), dict(hyperviscosity=(1e300, 8)), dict(hyperviscosity=(1e30, 8))):
        with pytest.raises(ValueError):
            mk(**bad)
    ok = mk(hyperviscosity=(1e-9, 8), hypofriction=(0.1, 4), beta=-3.0)
    assert ok._linear() and ok._lin.shape == (22, 64, 2) and ok._lin.dtype == np.float32 and ok.hyperviscosity == (1e-9, 8) and ok.beta == -3.0
    assert mk().hyperviscosity == (0.0, 2) and mk().hypofriction == (0.0, 1) and not mk()._linear() and mk(beta=-1e-9)._linear()
    lam = ok.linear_operator()
    assert lam.dtype == np.complex128 and lam.shape == (22, 64) and lam[0, 0] == 0 and np.all(lam[:, 22:43] == 0) and lam[0, 1].imag == -3.0

    L = _lib.lib()
    nb, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.nns_spec_ns_workspace(3, 64, 64, ctypes.byref(nb)) == 0 and L.nns_spec_ns_scalar_workspace(3, 64, 64, ctypes.byref(ns)) == 0
    what = torch.zeros(3, 22, 64, 2, device='cuda')
    that = torch.zeros(3, 22, 64, 2, device='cuda')
    mean = torch.zeros(3, 2, device='cuda')
    work = torch.empty(ns.value, dtype=torch.uint8, device='cuda')
    lin = torch.zeros(22, 64, 2, device='cuda')
    lin[..., 0] = -0.01
    amp = torch.zeros(22, 64, device='cuda')
    amp[2, 3] = 1.0
    clock = torch.zeros(1, dtype=torch.int64, device='cuda')
    ids = torch.arange(3, dtype=torch.int32, device='cuda')
    what[:, 1, 1, 0] = that[:, 1, 1, 1] = 1.0
    w0, t0 = what.clone(), that.clone()
    p = lambda t: t.data_ptr()

    def step(t=p(that), l=p(lin), a=None, c=None, i=None, wb=ns.value, nx=64, dt=0.01, kappa=0.1, bx=0.3, nsteps=1, batch=3):
        return L.nns_spec_ns_step_linear_f32(p(what), t, p(mean), None, 0, p(work), wb, batch, nx, 64, TWO_PI, TWO_PI, dt, kappa, 0.5, 0.5, bx, 1.2,
                                             l, a, 12345, c, i, nsteps, None)
    assert step(l=None) == INVALID and b'lin' in L.nns_last_error()
    assert step(a=p(amp)) == INVALID and b'amp' in L.nns_last_error()
    assert step(a=p(amp), c=p(clock)) == INVALID and step(c=p(clock), i=p(ids)) == INVALID and step(i=p(ids)) == INVALID
    assert step(wb=ns.value - 1) == WORKSPACE and b'nns_spec_ns_scalar_workspace' in L.nns_last_error()
    assert step(t=None, wb=nb.value - 1) == WORKSPACE and b'nns_spec_ns_workspace' in L.nns_last_error()
    assert step(nx=96) == UNSUPPORTED and step(dt=0.0) == INVALID and step(nsteps=-1) == INVALID and step(batch=0) == INVALID
    assert step(kappa=-1.0) == INVALID and step(bx=math.nan) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(what, w0) and torch.equal(that, t0) and int(clock) == 0     # nothing was launched
    assert step(nsteps=0) == 0
    assert step() == 0 and step(t=None, wb=nb.value, kappa=-1.0, bx=math.nan) == 0 and step(a=p(amp), c=p(clock), i=p(ids)) == 0
    torch.cuda.synchronize()
    assert int(clock) == 1 and not torch.equal(what, w0) and bool(torch.isfinite(what).all())
    # the spectrum entry
    rate = torch.full((22, 64), -1.0, dtype=torch.float64, device='cuda')
    S, dk = ops.spec_ns_shells(64, 64, TWO_PI, TWO_PI)
    out = torch.zeros(3, 2, S, dtype=torch.float64, device='cuda')

    def spec(w=p(what), r=p(rate), o=p(out), nshell=S, batch=3, nx=64, Lx=TWO_PI):
        return L.nns_spec_ns_linear_spectrum_f32(w, r, o, nshell, batch, nx, 64, Lx, TWO_PI, None)
    assert spec(w=None) == INVALID and spec(r=None) == INVALID and spec(o=None) == INVALID and spec(batch=0) == INVALID
    assert spec(nshell=S - 1) == INVALID and spec(nx=96) == UNSUPPORTED and spec(Lx=0.0) == INVALID
    assert spec() == 0
    # host refusals of the ops
    st = ok.init(torch.zeros(3, 64, 64, device='cuda'), torch.zeros(3, 64, 64, device='cuda'))
    args = lambda **kw: dict(dict(what=st.what, that=None, mean=st.mean, ghat=None, work=st.work, ny=64, Lx=TWO_PI, Ly=TWO_PI, dt=0.01, kappa=0.0,
                                  grad=(0.0, 0.0), buoyancy=(0.0, 0.0), lin=lin), **kw)
    for bad in (dict(lin=lin[:21]), dict(lin=lin[..., 0].contiguous()), dict(amp=amp), dict(amp=amp, clock=clock), dict(amp=amp, clock=clock, ids=ids[:2]),
                dict(amp=amp, clock=clock, ids=ids, seed=-1)):
        with pytest.raises(ValueError):
            ops.spec_ns_step_linear_(**args(**bad))
    for bad in (dict(lin=lin.double()), dict(lin=lin.cpu()), dict(lin=None), dict(amp=amp, clock=clock.int(), ids=ids), dict(amp=amp, clock=clock, ids=ids, seed=1.0)):
        with pytest.raises(TypeError):
            ops.spec_ns_step_linear_(**args(**bad))
    with pytest.raises(_lib.NnsError, match='workspace'):
        ops.spec_ns_step_linear_(**args(work=st.work[:-1]))
    with pytest.raises(TypeError):
        ops.spec_ns_linear_spectrum(st.what, rate.float(), 64, TWO_PI, TWO_PI)
    with pytest.raises(ValueError):
        ops.spec_ns_linear_spectrum(st.what, rate[:21], 64, TWO_PI, TWO_PI)
