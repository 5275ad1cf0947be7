"""GPU checks of the passive scalar of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip: nns_spec_ns_step_scalar_f32,
nns_spec_ns_scalar_*, through nns.periodic.PeriodicSolver with kappa) against the flow-only step (bitwise), the float64 restatement
tests/pspec_scalar_oracle.py and the analytic advected sine."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pspec_cases as C
import pspec_forced_cases as FC
import pspec_scalar_cases as SC
import pspec_scalar_oracle as SO
from conftest import rel_l2

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi
IDS = [C.case_id(c) for c in SC.CASES]


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device='cuda')          # a copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy().astype(np.float64)


def state_c(t):
    w = host(t)
    return w[..., 0] + 1j * w[..., 1]


def solver(nx, ny, dt, Lx=TWO_PI, Ly=TWO_PI, forced=True, kappa=SC.KAPPA, grad=SC.GRAD, nu=C.NU):
    from nns.periodic import PeriodicSolver
    s = PeriodicSolver(nx, ny, dt, C.RHO, nu, Lx=Lx, Ly=Ly, drag=FC.DRAG if forced else 0.0, kappa=kappa, scalar_gradient=grad)
    return s.kolmogorov_forcing(FC.KF, FC.AMP) if forced else s


def case_run(case, forced=True, nsteps=SC.NSTEPS, **kw):
    """(solver, state) of a case after nsteps steps with its scalar."""
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0 = SC.reference(case)[:4]
    s = solver(nx, ny, S.dt, Lx, Ly, forced, **kw)
    st = s.init(dev(u0), dev(v0), dev(th0))
    s.step(st, nsteps)
    return s, st


# ---------------------------------------------------------------------------------------------------- 1. passive, bitwise
@pytest.mark.parametrize('forced', [False, True], ids=['unforced', 'forced'])
@pytest.mark.parametrize('case', [SC.CASES[0], SC.CASES[3], SC.CASES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_the_flow_under_a_scalar_is_bitwise_the_flow_alone(gpu_device, case, forced):
    from nns import ops
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0 = SC.reference(case)[:4]
    s = solver(nx, ny, S.dt, Lx, Ly, forced)
    st = s.init(dev(u0), dev(v0), dev(th0))
    alone = s.init(dev(u0), dev(v0))
    assert alone.that is None and torch.equal(alone.what, st.what)
    assert st.work.numel() == ops.spec_ns_scalar_workspace(B, nx, ny) and alone.work.numel() == ops.spec_ns_workspace(B, nx, ny)
    s.step(st, SC.NSTEPS)
    if forced:
        ops.spec_ns_step_forced_(alone.what, alone.mean, s.ghat, alone.work, ny, Lx, Ly, S.dt, C.NU, FC.DRAG, SC.NSTEPS)
    else:
        ops.spec_ns_step_(alone.what, alone.mean, alone.work, ny, Lx, Ly, S.dt, C.NU, SC.NSTEPS)
    assert torch.equal(st.what, alone.what)
    assert float(st.what.abs().max()) > 0 and float(st.that.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 2. against the float64 restatement
@pytest.mark.parametrize('case', SC.CASES, ids=IDS)
def test_full_band_scalar_step_against_the_oracle(gpu_device, case):
    # the full-band inputs, dt rule, NSTEPS, NU, Kolmogorov force and drag of tests/test_gpu_pspec_forced.py, with a scalar that fills the band
    # (kappa 2e-3, G = (0.7, -0.4)).  The scalar's spectrum passes through the sequence of transforms and updates the vorticity's does, so its
    # bound is the project's bound for a state spectrum, C.BOUND_W, on the spectrum without its (0, 0) mode and on the fluctuation field.  A wrong
    # diffusivity, an ignored gradient or a dragged scalar is >= 100x that away on every case, a frozen velocity or a mask one mode too wide at
    # 64 x 64 (tests/test_oracle_pspec_scalar.py).  The mean of theta: 48 stage updates of a float32 value <= 0.5, 2^-24 relative each, worst
    # case 48 * 0.5 * 6e-8 = 1.4e-6; bound 3e-6.
    # measured on the MI355X (that', theta', |mean - oracle's|): 64x64 3.6e-7 3.6e-7 8.8e-8; 128x512 3.3e-7 3.9e-7 5.8e-11; 512x128 4.7e-7 4.9e-7
    # 6.0e-11; 1024x64 3.3e-7 3.8e-7 5.3e-11; 64x1024 3.3e-7 3.8e-7 3.4e-11 (only 64x64 has a mean flow to move the mean); u, v, p, what: the
    # figures of tests/test_gpu_pspec_forced.py (64x64 1.8e-7 2.1e-7 9.7e-7 2.6e-7 ... 64x1024 3.1e-7 6.2e-7 1.2e-6 2.8e-7)
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0, w, t, mean = SC.reference(case)
    s, st = case_run(case)
    n = nx * ny
    got_t = state_c(st.that)
    et = SC.rel_l2c(S.compact(S.fluctuation(S.expand(got_t))), S.compact(S.fluctuation(t)))
    th, ref_th = host(s.scalar(st)), S.scalar_field(t)
    fluct = lambda a: a - a.mean(axis=(-2, -1), keepdims=True)
    ef = rel_l2(fluct(th), fluct(ref_th))
    em = np.abs(got_t[:, 0, 0].real / n - t[..., 0, 0].real / n).max()
    got = [host(f) for f in s.fields(st)]
    errs = [rel_l2(g, r) for g, r in zip(got, S.fields(w, mean))]
    ew = SC.rel_l2c(state_c(st.what), S.compact(w))
    print('scalar full band %dx%d B=%d dt=%.2e, %d steps: rel-L2 that\' %.2e, theta\' %.2e, |mean - oracle\'s| %.2e (mean %s); u, v, p %s, what %.2e'
          % (nx, ny, B, S.dt, SC.NSTEPS, et, ef, em, got_t[:, 0, 0].real / n, ['%.2e' % e for e in errs], ew))
    assert et <= C.BOUND_W and ef <= C.BOUND_W, (et, ef)
    assert em <= 3e-6, em
    assert np.abs(th.mean(axis=(-2, -1)) - t[..., 0, 0].real / n).max() <= 3e-6
    assert max(errs[:2]) <= C.BOUND_UV and errs[2] <= C.BOUND_P and ew <= C.BOUND_W, (errs, ew)


@pytest.mark.parametrize('case', SC.CASES, ids=IDS)
def test_scalar_init_then_field_reproduces_a_band_limited_input(gpu_device, case):
    # no steps: rfft2, mask, compaction, expansion, irfft2; the bound of init / fields in tests/test_gpu_pspec.py
    # measured on the MI355X (field, spectrum): 1.1e-7 7.1e-8; 1.4e-7 8.0e-8; 1.5e-7 9.0e-8; 1.4e-7 8.6e-8; 1.4e-7 6.9e-8
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0 = SC.reference(case)[:4]
    s = solver(nx, ny, S.dt, Lx, Ly)
    st = s.init(dev(u0), dev(v0), dev(th0))
    e = rel_l2(host(s.scalar(st)), th0)
    et = SC.rel_l2c(state_c(st.that), S.compact(S.init_scalar(th0)))
    print('scalar init / field %dx%d: field rel-L2 %.2e, spectrum rel-L2 %.2e' % (nx, ny, e, et))
    assert e <= 1e-6 and et <= 1e-6, (e, et)
    assert tuple(st.that.shape) == (B, s.my1, nx, 2)
    # a mode outside the band is dropped, the mean is kept
    x = np.arange(nx)[:, None] / nx
    rough = (np.cos(TWO_PI * (nx // 3 + 1) * x) + np.zeros((nx, ny)) + 0.25).astype(np.float32)
    st2 = s.init(dev(u0[0]), dev(v0[0]), dev(rough))
    assert np.abs(host(s.scalar(st2)) - 0.25).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------- 3. the advected sine, 200 steps
@pytest.mark.parametrize('sine', SC.SINES, ids=['%dx%d' % s[:2] for s in SC.SINES])
def test_advected_sine_200_steps(gpu_device, sine):
    # tests/test_oracle_pspec_scalar.py::test_advected_sine_under_a_uniform_flow on the GPU: the scheme's own error is <= 4e-8 of the amplitude,
    # so what is measured is float32.  Bound: the project's 200-step analytic bound, 2e-6 of the decayed amplitude; the mean and gradient of
    # the solution are sized in pspec_scalar_cases.py so that the float32 drift of a mean under a constant source stays below a quarter of it.
    # measured on the MI355X: 8.4e-7 (64x64), 9.7e-7 (256x1024, Ly = 4 pi), 1.5e-6 (1024x64, Lx = 1)
    nx, ny, Lx, Ly, m, U, kappa, dt = sine
    n = SC.SINE_STEPS
    s = solver(nx, ny, dt, Lx, Ly, forced=False, kappa=kappa, grad=SC.SINE_GRAD, nu=0.01)
    th0, _ = SO.advected_sine(nx, ny, 0.0, m, U, kappa, SC.SINE_GRAD, SC.SINE_MEAN, Lx, Ly)
    st = s.init(dev(np.full((nx, ny), U[0])), dev(np.full((nx, ny), U[1])), dev(th0))
    s.step(st, n)
    ref, amp = SO.advected_sine(nx, ny, n * dt, m, U, kappa, SC.SINE_GRAD, SC.SINE_MEAN, Lx, Ly)
    err = np.abs(host(s.scalar(st))[0] - ref).max() / amp
    print('advected sine %dx%d m %s, %d steps: max error / decayed amplitude %.2e (amplitude %.3f)' % (nx, ny, m, n, err, amp))
    assert float(st.what.abs().max()) == 0.0
    assert amp >= 0.5 and err <= 2e-6, (err, amp)


# ---------------------------------------------------------------------------------------------------- 4. bitwise invariants
def test_batch_members_are_the_single_runs_and_runs_repeat(gpu_device):
    case = SC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0 = SC.reference(case)[:4]
    s, st = case_run(case)
    _, again = case_run(case)
    assert torch.equal(st.what, again.what) and torch.equal(st.that, again.that)
    both = s.scalar(st)
    for k in range(B):
        one = s.init(dev(u0[k]), dev(v0[k]), dev(th0[k]))
        s.step(one, SC.NSTEPS)
        assert torch.equal(one.that[0], st.that[k]) and torch.equal(one.what[0], st.what[k])
        assert torch.equal(s.scalar(one)[0], both[k])
    c = st.clone()
    assert c.that is not st.that and torch.equal(c.that, st.that) and c.work.numel() == st.work.numel()
    s.step(c, 1)
    assert not torch.equal(c.that, st.that)


def test_graph_replay_of_a_scalar_run_is_bitwise_the_eager_loop(gpu_device):
    nx, ny, B = 64, 128, 2
    u0, v0, dt = C.full_band_input(nx, ny, B, TWO_PI, TWO_PI, (0.1, 0.2))
    th0 = SC.scalar_input(nx, ny, B, TWO_PI, TWO_PI, None)
    s = solver(nx, ny, dt)
    eager = s.simulate(dev(u0), dev(v0), 12, save_every=3, use_graph=False, theta0=dev(th0))
    assert s.last_simulate_used_graph is False
    graphed = s.simulate(dev(u0), dev(v0), 12, save_every=3, use_graph=True, theta0=dev(th0))
    assert s.last_simulate_used_graph is True
    assert len(eager) == 4 and len(graphed) == 4
    for a, b in zip(eager, graphed):
        assert a.shape == (5, B, nx, ny) and torch.equal(a, b)
    st = s.init(dev(u0), dev(v0), dev(th0))
    s.step(st, 12)
    assert torch.equal(eager[3][-1], s.scalar(st))
    assert not torch.equal(eager[3][0], eager[3][-1])
    # without theta0 a solver built with kappa is the solver built without it
    from nns.periodic import PeriodicSolver
    plain = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, drag=FC.DRAG).kolmogorov_forcing(FC.KF, FC.AMP)
    a, b = s.simulate(dev(u0), dev(v0), 12, save_every=3), plain.simulate(dev(u0), dev(v0), 12, save_every=3)
    assert len(a) == 3 and len(b) == 3
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a, eager):                                      # and the flow's frames are those of the run with the scalar
        assert torch.equal(x, y)


def test_zero_gradient_and_zero_diffusivity_are_accepted(gpu_device):
    case = SC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0 = SC.reference(case)[:4]
    Z = SC.scheme(nx, ny, S.dt, Lx, Ly, kappa=0.0, grad=(0.0, 0.0))
    w, t, mean = SC.oracle_run(Z, u0, v0, th0)
    s, st = case_run(case, kappa=0.0, grad=(0.0, 0.0))
    et = SC.rel_l2c(state_c(st.that), Z.compact(t))
    print('kappa = 0, G = 0, %dx%d: rel-L2 of that against the oracle %.2e' % (nx, ny, et))          # measured on the MI355X: 1.3e-7
    assert et <= C.BOUND_W, et
    # pure advection without a gradient conserves the mean of the scalar
    n = nx * ny
    assert np.abs(state_c(st.that)[:, 0, 0].real / n - Z.init_scalar(th0)[:, 0, 0].real / n).max() <= 3e-6


# ---------------------------------------------------------------------------------------------------- 5. diagnostics
@pytest.mark.parametrize('case', [SC.CASES[0], SC.CASES[2]], ids=[IDS[0], IDS[2]])
def test_scalar_diagnostics_against_the_oracle(gpu_device, case):
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0, w, t, mean = SC.reference(case)
    s, st = case_run(case)
    d = s.scalar_diagnostics(st)
    assert d._fields == ('variance', 'dissipation', 'flux_x', 'flux_y')
    assert all(x.dtype == torch.float64 and tuple(x.shape) == (B,) for x in d)
    got = [x.cpu().numpy() for x in d]
    # (a) against the restatement's numbers of its own state: the states' errors (BOUND_W, relative) twice in the quadratic variance and
    # dissipation, doubled again for margin: 4 BOUND_W relative.  The fluxes <u theta'> are bilinear: |d flux| <= |du| |theta'| + |u| |d theta'|
    # (Cauchy-Schwarz), so their error is taken relative to rms(u') rms(theta') = sqrt(2 E 2 variance), same bound.
    # measured on the MI355X (variance, dissipation, flux_x, flux_y): 64x64 6.7e-7 1.6e-7 1.7e-7 5.7e-8; 512x128 3.9e-7 2.5e-7 1.1e-8 6.8e-9
    ref = S.scalar_diag(w, t)
    fscale = np.sqrt(2 * S.diag(w)[0] * 2 * ref[0])
    ea = [np.abs(got[0] / ref[0] - 1).max(), np.abs(got[1] / ref[1] - 1).max(), (np.abs(got[2] - ref[2]) / fscale).max(),
          (np.abs(got[3] - ref[3]) / fscale).max()]
    # (b) against the restatement's sums over the GPU state copied to the host: isolates the reduction.  Bound 1e-6 relative (a float32
    # 1 / |k|^2 and float32 products would give 6e-8 each); the kernel forms them in float64.  measured on the MI355X: <= 1.1e-14
    own = S.scalar_diag(S.expand(state_c(st.what)), S.expand(state_c(st.that)))
    eb = [np.abs(g / r - 1).max() for g, r in zip(got, own)]
    print('scalar diagnostics %dx%d B=%d: %s; vs oracle state (variance, dissipation rel; fluxes / (rms u rms theta)) %s; vs oracle sums of the GPU '
          'state %s' % (nx, ny, B, [list(g) for g in got], ['%.2e' % e for e in ea], ['%.2e' % e for e in eb]))
    assert max(ea) <= 4 * C.BOUND_W, ea
    assert max(eb) <= 1e-6, eb
    assert min(np.abs(ref[2]).min(), np.abs(ref[3]).min()) >= 1e-3 * fscale.max()          # the fluxes are there to be compared
    # they repeat bitwise and each is the single-grid run's
    for a, b in zip(d, s.scalar_diagnostics(st)):
        assert torch.equal(a, b)
    k = B - 1
    one = s.init(dev(u0[k]), dev(v0[k]), dev(th0[k]))
    s.step(one, SC.NSTEPS)
    for a, b in zip(s.scalar_diagnostics(one), d):
        assert torch.equal(a[0], b[k])


# ---------------------------------------------------------------------------------------------------- 6. error codes
def test_error_codes(gpu_device):
    from nns import ops, _lib
    from nns.periodic import PeriodicSolver
    L = _lib.lib()
    n, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.nns_spec_ns_workspace(3, 64, 64, ctypes.byref(n)) == 0 and L.nns_spec_ns_scalar_workspace(3, 64, 64, ctypes.byref(ns)) == 0
    # the scalar step's 10 compacted fields (80 my1 bytes per row) stay below what fields() already needs (40 ny + 48), so on every supported
    # shape the two queries agree today; a flow-sized workspace is refused wherever they do not
    assert ns.value >= n.value > 0
    assert L.nns_spec_ns_scalar_workspace(0, 64, 64, ctypes.byref(ns)) == INVALID and L.nns_spec_ns_scalar_workspace(3, 64, 64, None) == INVALID
    assert L.nns_spec_ns_scalar_workspace(3, 96, 64, ctypes.byref(ns)) == UNSUPPORTED
    assert L.nns_spec_ns_scalar_workspace(3, 64, 64, ctypes.byref(ns)) == 0
    for B, nx, ny in ((1, 64, 64), (2, 1024, 64), (2, 64, 1024), (1, 1024, 1024)):
        assert ops.spec_ns_scalar_workspace(B, nx, ny) >= max(ops.spec_ns_workspace(B, nx, ny), 10 * B * nx * ops.spec_ns_kept_y(ny) * 8)
    what = torch.zeros(3, 22, 64, 2, device='cuda')
    that = torch.zeros(3, 22, 64, 2, device='cuda')
    mean = torch.zeros(3, 2, device='cuda')
    g = torch.zeros(3, 22, 64, 2, device='cuda')
    theta = torch.zeros(3, 64, 64, device='cuda')
    work = torch.empty(ns.value, dtype=torch.uint8, device='cuda')
    out = torch.empty(3, 4, dtype=torch.float64, device='cuda')
    p = lambda t: t.data_ptr()

    def step(gh=None, gb=0, drag=0.0, kappa=0.1, gx=0.5, gy=0.5, nx=64, wb=ns.value, w=p(what), t=p(that), batch=3, dt=0.01, nu=0.0, nsteps=1):
        return L.nns_spec_ns_step_scalar_f32(w, t, p(mean), gh, gb, p(work), wb, batch, nx, 64, TWO_PI, TWO_PI, dt, nu, drag, kappa, gx, gy,
                                             nsteps, None)
    assert step(w=None) == INVALID and step(t=None) == INVALID and step(batch=0) == INVALID
    assert step(kappa=-1e-3) == INVALID and b'kappa' in L.nns_last_error()
    assert step(kappa=math.nan) == INVALID and step(kappa=math.inf) == INVALID
    assert step(gx=math.nan) == INVALID and step(gy=math.inf) == INVALID
    assert step(p(g), 2) == INVALID and b'gbatch' in L.nns_last_error()
    assert step(None, 1) == INVALID and step(p(g), 0) == INVALID
    assert step(drag=-1.0) == INVALID and step(drag=math.nan) == INVALID
    assert step(dt=-0.01) == INVALID and step(nu=-1.0) == INVALID and step(nsteps=-1) == INVALID
    assert step(nx=96) == UNSUPPORTED
    assert step(wb=ns.value - 1) == WORKSPACE and b'nns_spec_ns_scalar_workspace' in L.nns_last_error()
    assert step(wb=n.value) == (WORKSPACE if ns.value > n.value else 0)
    assert step() == 0 and step(p(g), 3, 0.5) == 0 and step(p(g), 1) == 0 and step(drag=0.5) == 0 and step(kappa=0.0, gx=0.0, gy=0.0) == 0
    assert step(nsteps=0) == 0
    init = lambda th=p(theta), t=p(that), nx=64, wb=ns.value, batch=3: L.nns_spec_ns_scalar_init_f32(th, t, p(work), wb, batch, nx, 64, None)
    assert init(th=None) == INVALID and init(t=None) == INVALID and init(batch=0) == INVALID
    assert init(nx=96) == UNSUPPORTED and init(wb=ns.value - 1) == WORKSPACE and init() == 0
    field = lambda t=p(that), th=p(theta), nx=64, wb=ns.value: L.nns_spec_ns_scalar_field_f32(t, th, p(work), wb, 3, nx, 64, None)
    assert field(t=None) == INVALID and field(th=None) == INVALID and field(nx=96) == UNSUPPORTED and field(wb=ns.value - 1) == WORKSPACE
    assert field() == 0
    diag = lambda w=p(what), t=p(that), o=p(out), nx=64, kappa=0.1, Lx=TWO_PI: L.nns_spec_ns_scalar_diag_f32(w, t, o, 3, nx, 64, Lx, TWO_PI, kappa,
                                                                                                             None)
    assert diag(w=None) == INVALID and diag(t=None) == INVALID and diag(o=None) == INVALID
    assert diag(kappa=-1.0) == INVALID and diag(kappa=math.nan) == INVALID and diag(Lx=0.0) == INVALID
    assert diag(nx=96) == UNSUPPORTED and diag() == 0
    torch.cuda.synchronize()
    # host: refused before any launch
    z = torch.zeros(3, 64, 64, device='cuda')
    with pytest.raises(ValueError, match='kappa'):
        PeriodicSolver(64, 64, 0.01, 1.0, 0.0).init(z, z, theta=z)
    s = PeriodicSolver(64, 64, 0.01, 1.0, 0.0, kappa=0.1)
    with pytest.raises(TypeError):
        s.init(z, z, theta=z.double())
    with pytest.raises(ValueError):
        s.init(z, z, theta=torch.zeros(3, 64, 128, device='cuda'))
    with pytest.raises(ValueError):
        s.init(z, z, theta=torch.zeros(2, 64, 64, device='cuda'))
    st = s.init(z, z)
    with pytest.raises(ValueError, match='no scalar'):
        s.scalar(st)
    with pytest.raises(ValueError, match='no scalar'):
        s.scalar_diagnostics(st)
    sc = s.init(z, z, theta=z)
    with pytest.raises(ValueError):
        PeriodicSolver(64, 64, 0.01, 1.0, 0.0).step(sc)                # a state with a scalar on a solver without kappa
    with pytest.raises(ValueError):
        ops.spec_ns_step_scalar_(sc.what, sc.that[:2], sc.mean, None, sc.work, 64, TWO_PI, TWO_PI, 0.01, 0.0, 0.0, 0.1)
    with pytest.raises(TypeError):
        ops.spec_ns_step_scalar_(sc.what, sc.that.double(), sc.mean, None, sc.work, 64, TWO_PI, TWO_PI, 0.01, 0.0, 0.0, 0.1)
    with pytest.raises(_lib.NnsError, match='workspace'):
        ops.spec_ns_step_scalar_(sc.what, sc.that, sc.mean, None, sc.work[:-1], 64, TWO_PI, TWO_PI, 0.01, 0.0, 0.0, 0.1)
    with pytest.raises(ValueError):
        ops.spec_ns_scalar_diag(sc.what, sc.that, 64, TWO_PI, TWO_PI, 0.1, out=torch.empty(3, 3, dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError):
        ops.spec_ns_scalar_field(sc.that, sc.work, 128)
