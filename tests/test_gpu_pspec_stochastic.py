"""GPU checks of the white-in-time stochastic forcing of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_stochastic_f32, through nns.periodic.PeriodicSolver.set_stochastic_forcing / ring_forcing) against the restatement
tests/pspec_stochastic_oracle.py: the kick itself mode by mode, trajectories, the noise's bookkeeping (ids, clock, graph replay), the statistics
of the injection, and the paths that must stay bitwise what they are without the feature."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pspec_buoyant_cases as BC
import pspec_cases as C
import pspec_forced_cases as FC
import pspec_scalar_cases as SC
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


def ids_of(*k):
    return torch.tensor(k, dtype=torch.int32, device='cuda')


def rest_solver(nx=64, ny=64, Lx=TWO_PI, Ly=TWO_PI, dt=XC.REST_DT, ring=XC.REST_RING, rate=XC.REST_RATE, **kw):
    from nns.periodic import PeriodicSolver
    return PeriodicSolver(nx, ny, dt, C.RHO, 0.0, Lx=Lx, Ly=Ly, **kw).ring_forcing(rate, ring[0], ring[1], seed=XC.SEED)


def rest_state(s, B):
    z = torch.zeros(B, s.nx, s.ny, device='cuda')
    return s.init(z, z)


# ---------------------------------------------------------------------------------------------------- 1. one step from rest is the kick itself
@pytest.mark.parametrize('case', XC.KICKS, ids=XC.KICK_IDS)
def test_one_step_from_rest_is_the_kick(gpu_device, case):
    # N(0) = 0: after one step from rest what is sqrt(dt) a_k xi_k of the oracle on every forced stored mode, to XC.KICK_TOL relative to
    # a_k sqrt(dt) max(1, |xi_k|), and exactly 0 on every other element.  The same samples have the moments that
    # tests/test_oracle_pspec_stochastic.py records for the oracle's.
    # measured on the MI355X, worst error / tolerance: 64x64 0.105, 1024x64 0.122, 64x1024 0.117, 128x512 0.141, 1024x64 x 400 0.126 (2.8e-7
    # relative at worst: 4.7 float32 ulp); the moments are the oracle's recorded ones to their printed digits (profiles/pspec_stochastic_run.json)
    nx, ny, B, Lx, Ly = case
    amp = XC.kick_table(case)
    s = rest_solver(nx, ny, Lx, Ly, dt=XC.KICK_DT, ring=XC.kick_ring(*case), rate=XC.KICK_RATE)
    assert np.array_equal(s.stoch_amp, amp)
    st = rest_state(s, B)
    s.step(st, 1)
    mask, xi = XC.kick_samples(case)
    m = torch.as_tensor(mask, device='cuda')
    got = state_c(st.what[:, m])                                                   # [B, M]
    assert int(torch.count_nonzero(st.what[:, ~m])) == 0                           # nothing outside the ring, the (0, 0) mode included
    a = amp.astype(np.float64)[mask][None] * np.sqrt(XC.KICK_DT)
    err = np.abs(got - a * xi) / (XC.KICK_TOL * a * np.maximum(1.0, np.abs(xi)))
    m2, m1, bound = XC.moments(got / a)
    print('kick %s: %d forced stored modes x %d grids; worst error %.3f of the tolerance; mean |xi|^2 - 1 = %.3e, |mean xi| = %.3e (bound %.3e)'
          % (XC.KICK_IDS[XC.KICKS.index(case)], mask.sum(), B, err.max(), m2, m1, bound))
    assert err.max() <= 1.0, err.max()
    assert abs(m2) <= bound and m1 <= bound
    assert int(st.clock) == 1 and st.steps == 1


# ---------------------------------------------------------------------------------------------------- 2. the j = 0 line stays Hermitian
def test_kicks_keep_the_j0_line_hermitian(gpu_device):
    s = rest_solver()
    st = rest_state(s, 1)
    s.step(st, 1)
    line = st.what[0, 0]                                                           # [nx, 2]
    nx = s.nx
    assert int((line != 0).any(dim=1).sum()) == 6                                  # |m_x| = 4, 5, 6, both signs
    assert torch.equal(line[1:nx // 2, 0], line[nx // 2 + 1:, 0].flip(0)) and torch.equal(line[1:nx // 2, 1], -line[nx // 2 + 1:, 1].flip(0))
    # later steps: the deterministic step is Hermitian to rounding only (the defect printed is relative to the line's largest element;
    # measured on the MI355X: 2.5e-11 after 4 steps; the bound is 100 float32 ulp)
    s.step(st, 3)
    line = state_c(st.what[0, 0])
    defect = np.abs(line[1:nx // 2] - np.conj(line[:nx // 2:-1])).max() / np.abs(line).max()
    print('j = 0 line after 4 steps from rest: Hermitian defect %.2e of the largest element' % defect)
    assert defect <= 100 * 2.0 ** -24
    assert all(bool(torch.isfinite(f).all()) for f in s.fields(st))
    v = host(s.fields(st)[1])
    assert np.abs(v).max() > 0


# ---------------------------------------------------------------------------------------------------- 3. grid ids
def test_batch_members_are_the_single_runs_with_their_ids(gpu_device):
    nx, ny, B, Lx, Ly, _ = XC.TRAJ[0]
    assert (nx, ny, B) == (64, 64, 3)
    S, X, (u0, v0), _, _, _, rate, _ = XC.reference('flow', XC.TRAJ[0])
    s = traj_solver('flow', XC.TRAJ[0])
    st = s.init(dev(u0), dev(v0))
    assert st.noise_ids.tolist() == [0, 1, 2] and int(st.clock) == 0
    s.step(st, XC.NSTEPS)
    for k in range(B):
        one = s.init(dev(u0[k]), dev(v0[k]))
        one.noise_ids = ids_of(k)
        s.step(one, XC.NSTEPS)
        assert torch.equal(one.what[0], st.what[k])
    # equal ids and equal initial conditions: equal grids; different ids: different noise
    same = s.init(dev(u0[[0, 0, 0]]), dev(v0[[0, 0, 0]]))
    same.noise_ids = ids_of(7, 5, 7)
    s.step(same, XC.NSTEPS)
    assert torch.equal(same.what[0], same.what[2]) and not torch.equal(same.what[0], same.what[1])
    assert not torch.equal(same.what[0], st.what[0])


# ---------------------------------------------------------------------------------------------------- 4. clock, call pattern, graph replay
def test_eager_loop_one_call_many_calls_and_graph_replay_are_bitwise_equal(gpu_device):
    nx, ny, B = 64, 128, 2
    u0, v0, dt = C.full_band_input(nx, ny, B, TWO_PI, TWO_PI, (0.1, 0.2))
    from nns.periodic import PeriodicSolver
    s = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, drag=FC.DRAG).kolmogorov_forcing(FC.KF, FC.AMP).ring_forcing(2.0, 4, 6, seed=XC.SEED)
    eager = s.simulate(dev(u0), dev(v0), 12, save_every=1, use_graph=False)
    assert s.last_simulate_used_graph is False
    graphed = s.simulate(dev(u0), dev(v0), 12, save_every=1, use_graph=True)
    assert s.last_simulate_used_graph is True
    for a, b in zip(eager, graphed):
        assert a.shape == (13, B, nx, ny) and torch.equal(a, b)
    once, many = s.init(dev(u0), dev(v0)), s.init(dev(u0), dev(v0))
    s.step(once, 12)
    mid = None
    for k in range(12):
        s.step(many, 1)
        if k == 5:
            mid = many.clone()
            assert int(mid.clock) == 6 and mid.clock.data_ptr() != many.clock.data_ptr() and mid.noise_ids.data_ptr() != many.noise_ids.data_ptr()
    assert torch.equal(once.what, many.what)
    assert int(once.clock) == 12 and int(many.clock) == 12 and once.clock.dtype == torch.int64 and once.steps == 12
    for a, b in zip(s.fields(once), eager):
        assert torch.equal(a, b[12])
    s.step(mid, 6)                                                                 # the clone continues like its origin
    assert torch.equal(mid.what, many.what) and int(mid.clock) == 12
    # the steps differ from each other, and another seed gives another run
    assert not torch.equal(eager[0][1] - eager[0][0], eager[0][2] - eager[0][1])
    other = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, drag=FC.DRAG).kolmogorov_forcing(FC.KF, FC.AMP).ring_forcing(2.0, 4, 6, seed=XC.SEED + 1)
    assert not torch.equal(other.step(other.init(dev(u0), dev(v0)), 12).what, once.what)


# ---------------------------------------------------------------------------------------------------- 5. trajectories against the float64 oracle
def traj_solver(kind, case):
    from nns.periodic import PeriodicSolver
    nx, ny, B, Lx, Ly, _ = case
    S, X, ins, w, t, mean, rate, ratio = XC.reference(kind, case)
    kw = {} if kind == 'flow' else dict(kappa=SC.KAPPA, scalar_gradient=SC.GRAD)
    if kind == 'buoyant':
        kw['buoyancy'] = BC.BUOY
    s = PeriodicSolver(nx, ny, S.dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=FC.DRAG, **kw).kolmogorov_forcing(FC.KF, FC.AMP)
    s.ring_forcing(rate, *XC.traj_ring(nx, ny, Lx, Ly), seed=XC.SEED)
    assert np.array_equal(s.stoch_amp, X.amp)
    return s


@pytest.mark.parametrize('kind, case', [('flow', c) for c in XC.TRAJ] + [('scalar', XC.SCALAR_CASE), ('buoyant', XC.BUOYANT_CASE)],
                         ids=XC.TRAJ_IDS + ['64x64-scalar', '64x64-buoyant'])
def test_trajectory_against_the_oracle(gpu_device, kind, case):
    # NSTEPS steps of the full-band inputs under the Kolmogorov force and drag of pspec_forced_cases and a ring force whose kicks inject, in the
    # mean, the initial state's energy over the run (ratio printed: the noise is comparable to the state).  The kick adds rounding of a few ulp
    # of itself, so the bounds are those of the deterministic step: C.BOUND_W, C.BOUND_UV, C.BOUND_P.  Each mutation of the scheme is >= 1.2e4 x
    # BOUND_W away at 64 x 64 (tests/test_oracle_pspec_stochastic.py).
    # measured on the MI355X (what; u, v, p; that' with a scalar): 64x64 2.32e-7; 1.77e-7 2.06e-7 6.6e-7 -- 128x512 2.33e-7; 2.33e-7 2.28e-7 2.8e-6 --
    # 1024x64 2.47e-7; 2.08e-7 2.52e-7 1.9e-6 -- 64x64 scalar 2.32e-7; the flow's figures; that' 2.30e-7 -- 64x64 buoyant 2.35e-7; 1.77e-7 2.14e-7
    # 3.1e-7; that' 2.63e-7 (profiles/pspec_stochastic_run.json): the deterministic step's figures
    nx, ny, B, Lx, Ly, _ = case
    S, X, ins, w, t, mean, rate, ratio = XC.reference(kind, case)
    s = traj_solver(kind, case)
    st = s.init(*[dev(a) for a in ins])
    s.step(st, XC.NSTEPS)
    ew = SC.rel_l2c(state_c(st.what), S.compact(w))
    got = [host(f) for f in s.fields(st)]
    ref = S.fields(w, mean, t) if kind == 'buoyant' else S.fields(w, mean)
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    et = 0.0 if t is None else SC.rel_l2c(S.compact(S.fluctuation(S.expand(state_c(st.that)))), S.compact(S.fluctuation(t)))
    print('stochastic %s %dx%d B=%d dt=%.2e, %d steps, rate %.3g (injected / initial energy %.2f): rel-L2 what %.2e, that\' %.2e; u, v, p %s'
          % (kind, nx, ny, B, S.dt, XC.NSTEPS, rate, ratio, ew, et, ['%.2e' % e for e in errs]))
    assert 0.99 <= ratio <= 1.01
    assert ew <= C.BOUND_W and et <= C.BOUND_W, (ew, et)
    assert max(errs[:2]) <= C.BOUND_UV, errs
    assert errs[2] <= (BC.BOUND_P if kind == 'buoyant' else C.BOUND_P), errs
    assert int(st.clock) == XC.NSTEPS


# ---------------------------------------------------------------------------------------------------- 6. the injection, per shell
def test_per_shell_injection_from_rest(gpu_device):
    # nu = 0, from rest, 64 x 64, B = 64, 20 steps: the batch mean of spectrum().energy / t per ring shell against stochastic_injection(), within
    # 5 sampling standard deviations: a shell's energy is a sum of exponential variables of equal mean over its independent modes (N_s / 2: a
    # mode and its conjugate are one), so the batch mean has the relative standard deviation 1 / sqrt(B N_s / 2); the total likewise.  The
    # nonlinear term conserves the total and moves energy between the shells, by less than the sampling error in this short run from rest.
    # measured on the MI355X: shells 4, 5, 6 are 0.14, 0.77, 0.04 standard deviations off (3.1 %, 3.3 %, 2.8 % each), the total 0.55; 7e-4 of the
    # energy has left the ring
    B, nsteps = 64, 20
    s = rest_solver()
    st = rest_state(s, B)
    sp0 = s.spectrum(st)
    assert not bool(sp0.energy.any())
    s.step(st, nsteps)
    t = nsteps * s.dt
    inj = s.stochastic_injection()
    E = s.spectrum(st).energy.cpu().numpy().mean(axis=0) / t
    N = s.shell_mode_counts()
    ring = np.nonzero(inj)[0]
    assert list(ring) == [4, 5, 6] and abs(inj.sum() - XC.REST_RATE) <= 1e-6 * XC.REST_RATE
    sd = 1.0 / np.sqrt(B * N[ring] / 2.0)
    dev_s = (E[ring] / inj[ring] - 1) / sd
    dev_t = (E.sum() / inj.sum() - 1) * np.sqrt(B * N[ring].sum() / 2.0)
    print('injection from rest, B = %d, %d steps: ring shells %s of their standard deviations off (each %s relative); total %.2f off; outside the ring '
          '%.2e of the total' % (B, nsteps, ['%.2f' % d for d in dev_s], ['%.3f' % x for x in sd], dev_t, 1 - E[ring].sum() / E.sum()))
    assert np.abs(dev_s).max() <= 5 and abs(dev_t) <= 5
    budget = s.energy_budget(st)
    plain = rest_solver().set_stochastic_forcing(None).energy_budget(st)
    assert torch.equal(budget, plain + torch.from_numpy(inj).to(budget.device))


# ---------------------------------------------------------------------------------------------------- 7. untouched paths
@pytest.mark.parametrize('kind', ['unforced', 'forced', 'scalar', 'buoyant'])
def test_paths_without_a_stochastic_force_are_bitwise_what_they_are(gpu_device, kind):
    # a solver that never had a stochastic force and one whose force was removed again make the same calls, so they give the same bits
    # as each other; what those bits are is pinned by the sibling files' tests, which run unchanged
    from nns.periodic import PeriodicSolver
    case = SC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    u0, v0, dt = C.full_band_input(*case)
    th0 = SC.scalar_input(*case) if kind in ('scalar', 'buoyant') else None
    kw = {} if th0 is None else dict(kappa=SC.KAPPA, scalar_gradient=SC.GRAD)
    if kind == 'buoyant':
        kw['buoyancy'] = BC.BUOY

    def run(touch):
        s = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=0.0 if kind == 'unforced' else FC.DRAG, **kw)
        if kind != 'unforced':
            s.kolmogorov_forcing(FC.KF, FC.AMP)
        if touch:
            s.ring_forcing(1.0, 4, 6, seed=XC.SEED)
            s.set_stochastic_forcing(None)
        frames = s.simulate(dev(u0), dev(v0), 6, save_every=3, theta0=None if th0 is None else dev(th0))
        st = s.init(dev(u0), dev(v0), None if th0 is None else dev(th0))
        s.step(st, 6)
        assert st.clock is None and st.noise_ids is None
        return frames, st
    (fa, a), (fb, b) = run(False), run(True)
    assert len(fa) == len(fb) == (3 if th0 is None else 4)
    assert all(torch.equal(x, y) for x, y in zip(fa, fb))
    assert torch.equal(a.what, b.what) and (th0 is None or torch.equal(a.that, b.that))
    # and the stochastic force does change the run
    s = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=0.0 if kind == 'unforced' else FC.DRAG, **kw).ring_forcing(1.0, 4, 6, seed=XC.SEED)
    if kind != 'unforced':
        s.kolmogorov_forcing(FC.KF, FC.AMP)
    c = s.step(s.init(dev(u0), dev(v0), None if th0 is None else dev(th0)), 6)
    assert not torch.equal(c.what, a.what) and int(c.clock) == 6


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_error_codes(gpu_device):
    from nns import ops, _lib
    L = _lib.lib()
    nb, ns = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.nns_spec_ns_workspace(3, 64, 64, ctypes.byref(nb)) == 0 and L.nns_spec_ns_scalar_workspace(3, 64, 64, ctypes.byref(ns)) == 0
    what = torch.zeros(3, 22, 64, 2, device='cuda')
    that = torch.zeros(3, 22, 64, 2, device='cuda')
    mean = torch.zeros(3, 2, device='cuda')
    work = torch.empty(ns.value, dtype=torch.uint8, device='cuda')
    amp = torch.zeros(22, 64, device='cuda')
    amp[2, 3] = 1.0
    clock = torch.zeros(1, dtype=torch.int64, device='cuda')
    ids = torch.arange(3, dtype=torch.int32, device='cuda')
    what[:, 1, 1, 0] = that[:, 1, 1, 1] = 1.0
    w0, t0 = what.clone(), that.clone()
    p = lambda t: t.data_ptr()

    def step(t=p(that), a=p(amp), c=p(clock), i=p(ids), wb=ns.value, nx=64, dt=0.01, kappa=0.1, bx=0.3, nsteps=1, batch=3, drag=0.0):
        return L.nns_spec_ns_step_stochastic_f32(p(what), t, p(mean), None, 0, p(work), wb, batch, nx, 64, TWO_PI, TWO_PI, dt, 0.0, drag, kappa, 0.5,
                                                 0.5, bx, 1.2, a, 12345, c, i, nsteps, None)
    assert step(a=None) == INVALID and b'amp' in L.nns_last_error()
    assert step(c=None) == INVALID and step(i=None) == INVALID
    assert step(wb=ns.value - 1) == WORKSPACE and b'nns_spec_ns_scalar_workspace' in L.nns_last_error()
    assert step(t=None, wb=nb.value - 1) == WORKSPACE and b'nns_spec_ns_workspace' in L.nns_last_error()
    assert step(nx=96) == UNSUPPORTED and step(dt=0.0) == INVALID and step(nsteps=-1) == INVALID and step(batch=0) == INVALID
    assert step(kappa=-1.0) == INVALID and step(bx=math.nan) == INVALID and step(drag=-1.0) == INVALID
    torch.cuda.synchronize()
    # nothing was launched: every buffer is as it was, the clock included
    assert torch.equal(what, w0) and torch.equal(that, t0) and int(clock) == 0
    assert step(nsteps=0) == 0 and int(clock) == 0
    assert step() == 0 and step(t=None, wb=nb.value) == 0 and step(t=None, wb=nb.value, kappa=-1.0, bx=math.nan) == 0       # no scalar: its numbers are ignored
    torch.cuda.synchronize()
    assert int(clock) == 3 and not torch.equal(what, w0)
    # host refusals of the op and of the solver
    s = rest_solver()
    st = rest_state(s, 3)
    args = lambda **kw: dict(dict(what=st.what, that=None, mean=st.mean, ghat=None, work=st.work, ny=64, Lx=TWO_PI, Ly=TWO_PI, dt=0.01, nu=0.0, drag=0.0,
                                  kappa=0.0, grad=(0.0, 0.0), buoyancy=(0.0, 0.0), amp=amp, seed=1, clock=clock, ids=ids), **kw)
    for bad in (dict(amp=amp[:21]), dict(amp=amp.t().contiguous()), dict(ids=ids[:2]), dict(clock=torch.zeros(2, dtype=torch.int64, device='cuda')),
                dict(seed=-1), dict(seed=2 ** 64), dict(amp=amp[:, :32].contiguous())):
        with pytest.raises(ValueError):
            ops.spec_ns_step_stochastic_(**args(**bad))
    for bad in (dict(amp=amp.double()), dict(ids=ids.long()), dict(clock=clock.int()), dict(ids=ids.cpu()), dict(clock=None), dict(seed=1.0),
                dict(seed=True)):
        with pytest.raises(TypeError):
            ops.spec_ns_step_stochastic_(**args(**bad))
    with pytest.raises(_lib.NnsError, match='workspace'):
        ops.spec_ns_step_stochastic_(**args(work=st.work[:-1]))
    st.noise_ids = ids_of(0, 1)
    with pytest.raises(ValueError, match='ids'):
        s.step(st, 1)
    st.noise_ids = None
    s.step(st, 1)                                                                  # made on first use
    assert st.noise_ids.tolist() == [0, 1, 2] and int(st.clock) == 1
