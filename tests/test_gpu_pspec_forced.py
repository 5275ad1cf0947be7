"""GPU checks of the forced, damped step and the diagnostics of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip:
nns_spec_ns_step_forced_f32, nns_spec_ns_diag_f32, through nns.periodic.PeriodicSolver) against the unforced step (bitwise), the float64
restatement tests/pspec_forced_oracle.py, analytic solutions and the spectral residual engine."""
import ctypes
import math

import numpy as np
import pytest
import torch

import pspec_cases as C
import pspec_forced_cases as FC
import pspec_forced_oracle as F
import pspec_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(ts):
    return [t.cpu().numpy().astype(np.float64) for t in ts]


def solver(nx, ny, dt, rho, nu, Lx=TWO_PI, Ly=TWO_PI, drag=0.0):
    from nns.periodic import PeriodicSolver
    return PeriodicSolver(nx, ny, dt, rho, nu, Lx=Lx, Ly=Ly, drag=drag)


def state_c(t):
    w = t.cpu().numpy().astype(np.float64)
    return w[..., 0] + 1j * w[..., 1]


def run(s, u0, v0, nsteps):
    st = s.init(dev(u0), dev(v0))
    s.step(st, nsteps)
    return host(s.fields(st)), st


# ---------------------------------------------------------------------------------------------------- 1. the unforced path is untouched
@pytest.mark.parametrize('nx,ny,B,mean', [(1024, 64, 1, (0.0, 0.0)), (64, 1024, 1, (0.0, 0.0)), (128, 256, 3, (0.2, 0.1))])
def test_forced_entry_without_force_and_drag_is_bitwise_the_unforced_step(gpu_device, nx, ny, B, mean):
    from nns import ops
    u0, v0 = O.random_ic(B, nx, ny, 8, seed=nx + ny, umax=1.5, mean=mean)
    s = solver(nx, ny, 0.005, 1.0, 0.005)
    a = s.init(dev(u0), dev(v0))
    b = a.clone()
    ops.spec_ns_step_(a.what, a.mean, a.work, ny, s.Lx, s.Ly, s.dt, s.nu, 12)
    ops.spec_ns_step_forced_(b.what, b.mean, None, b.work, ny, s.Lx, s.Ly, s.dt, s.nu, 0.0, 12)
    assert torch.equal(a.what, b.what)
    assert float(a.what.abs().max()) > 0


def test_solver_without_force_takes_the_unforced_path_before_and_after_a_force(gpu_device):
    nx, ny = 64, 128
    u0, v0 = O.random_ic(2, nx, ny, 6, seed=5, umax=1.0)
    s = solver(nx, ny, 0.01, 1.0, 0.01, drag=0.0)
    before = s.simulate(dev(u0), dev(v0), 12, save_every=3)
    s.kolmogorov_forcing(4, 2.0)
    forced = s.simulate(dev(u0), dev(v0), 12, save_every=3)
    assert s.set_forcing(None) is s and s.ghat is None
    after = s.simulate(dev(u0), dev(v0), 12, save_every=3)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert not torch.equal(before[0], forced[0])
    plain = solver(nx, ny, 0.01, 1.0, 0.01).simulate(dev(u0), dev(v0), 12, save_every=3)       # and they are what a solver built without
    for a, b in zip(before, plain):                                                             # the argument gives
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- 2. against the float64 restatement
def _against_the_oracle(label, case, S, s, u0, v0):
    nx, ny, B, Lx, Ly, mean = case
    w, ref = FC.oracle_run(S, u0, v0)
    st = s.init(dev(u0), dev(v0))
    s.step(st, C.NSTEPS)
    got = host(s.fields(st))
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    ew = rel_l2(state_c(st.what), S.compact(w))
    # the force spectrum in force space (g^ / |k|: by Parseval the rel-L2 of f_s), where the 1e-6 of init / fields in tests/test_gpu_pspec.py
    # applies; g^ itself weighs the float32 transform's rounding noise by |k| / k_force (2.0e-6 for the k = 4 sine at ny = 1024)
    ik = np.sqrt(S.compact(S.ik2 + 0j).real)
    eg = rel_l2(state_c(s.ghat) * ik, S.compact(S.g) * ik)
    print('%s %dx%d B=%d dt=%.2e, %d steps: rel-L2 u, v, p %s, what %.2e, ghat / |k| %.2e'
          % (label, nx, ny, B, S.dt, C.NSTEPS, ['%.2e' % e for e in errs], ew, eg))
    assert max(errs[:2]) <= C.BOUND_UV and errs[2] <= C.BOUND_P and ew <= C.BOUND_W, (errs, ew)
    assert eg <= 1e-6, eg
    assert np.abs(st.mean.cpu().numpy() - np.array(mean)).max() <= 1e-6          # the mean flow is neither forced nor damped


@pytest.mark.parametrize('case', C.FULL_BAND, ids=[C.case_id(c) for c in C.FULL_BAND])
def test_kolmogorov_forced_full_band_step_against_the_oracle(gpu_device, case):
    # the inputs, dt rule, NSTEPS and NU of tests/test_gpu_pspec_edges.py's full-band cases under a shared Kolmogorov force (k = 4, A = 2)
    # and drag 1; bounds of pspec_cases.py as they stand.  A build that ignores the force, the drag, or forces stage 1 only is >= 100x
    # BOUND_UV away (tests/test_oracle_pspec_forced.py::test_forced_cases_detect_an_ignored_force_drag_or_stage).
    # measured on the MI355X (u, v, p, what): 64x64 1.8e-7 2.1e-7 9.7e-7 2.5e-7; 128x512 2.7e-7 2.8e-7 7.3e-6 2.5e-7;
    # 512x128 2.7e-7 2.9e-7 7.2e-6 2.5e-7; 512x512 2.9e-7 3.0e-7 7.2e-6 2.7e-7; 256x1024 2.8e-7 3.4e-7 3.0e-6 2.7e-7;
    # 1024x256 2.7e-7 2.9e-7 3.3e-6 2.8e-7; 1024x64 2.3e-7 2.9e-7 1.7e-6 2.8e-7; 64x1024 3.1e-7 6.2e-7 1.2e-6 2.8e-7: the unforced figures
    nx, ny, B, Lx, Ly, mean = case
    u0, v0, dt = C.full_band_input(*case)
    S = FC.scheme(nx, ny, dt, Lx, Ly).kolmogorov_forcing(FC.KF, FC.AMP)
    s = solver(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG).kolmogorov_forcing(FC.KF, FC.AMP)
    assert tuple(s.ghat.shape) == (1, s.my1, nx, 2)
    _against_the_oracle('Kolmogorov-forced full band', case, S, s, u0, v0)


def test_per_grid_forces_against_the_oracle(gpu_device):
    # three different random forces filling the band, one per grid.  measured on the MI355X (u, v, p, what): 1.8e-7 2.1e-7 1.4e-6 2.4e-7
    case = (64, 64, 3, TWO_PI, TWO_PI, (0.3, -0.2))
    nx, ny, B, Lx, Ly, mean = case
    u0, v0, dt = C.full_band_input(*case)
    fx, fy = FC.random_forces(B, nx, ny, 21, Lx, Ly)
    S = FC.scheme(nx, ny, dt, Lx, Ly).set_forcing(fx, fy)
    s = solver(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG).set_forcing(fx, fy)
    assert tuple(s.ghat.shape) == (B, s.my1, nx, 2)
    _against_the_oracle('per-grid forces', case, S, s, u0, v0)
    w_shared, _ = FC.oracle_run(FC.scheme(nx, ny, dt, Lx, Ly).set_forcing(fx[:1], fy[:1]), u0, v0)
    assert rel_l2(S.compact(w_shared)[1:], S.compact(FC.oracle_run(S, u0, v0)[0])[1:]) >= 100 * C.BOUND_W     # grid k does see force k


def test_a_rough_force_is_projected_against_the_oracle(gpu_device):
    # a force that is neither solenoidal nor band-limited nor zero-mean: only f_s acts, and forcing_fields() returns it.
    # measured on the MI355X (u, v, p, what): 2.9e-7 3.0e-7 4.1e-6 2.5e-7; forcing_fields against the oracle's: 2.0e-7, 1.8e-7
    case = (128, 512, 2, 1.0, 4.0, (0.0, 0.0))
    nx, ny, B, Lx, Ly, mean = case
    u0, v0, dt = C.full_band_input(*case)
    fx, fy = FC.rough_force(nx, ny, 31)
    S = FC.scheme(nx, ny, dt, Lx, Ly).set_forcing(fx, fy)
    s = solver(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG).set_forcing(fx[0], fy[0])          # [nx, ny]: shared
    _against_the_oracle('rough force', case, S, s, u0, v0)
    fs = host(s.forcing_fields())
    ref = S.forcing_fields()
    errs = [rel_l2(g, r) for g, r in zip(fs, ref)]
    print('forcing_fields rel-L2 vs the oracle:', ['%.2e' % e for e in errs])
    assert fs[0].shape == (1, nx, ny) and max(errs) <= 1e-6, errs           # the bound of init / fields in tests/test_gpu_pspec.py
    assert rel_l2(fs[0], fx.astype(np.float64)) > 0.1                        # the projection removed a real part of the force


# ---------------------------------------------------------------------------------------------------- 3. analytic solutions, 200 steps
@pytest.mark.parametrize('nx,ny,Ly,U0,drag', [(64, 64, TWO_PI, 0.0, 0.0), (256, 1024, TWO_PI, 0.5, 0.5), (1024, 256, 2 * TWO_PI, 0.0, 0.5)])
def test_laminar_kolmogorov_200_steps(gpu_device, nx, ny, Ly, U0, drag):
    # from u = (U0, 0) under f = (A sin(k y), 0): u = U0 + A / lam (1 - exp(-lam t)) sin(k y), v = 0 (pspec_forced_oracle.kolmogorov_laminar).
    # RK4's quadrature error of the constant force is n (lam dt)^5 / 2880 <= 1e-12 of the amplitude here: what is measured is float32.
    # Expectation: the 2e-6 of test_taylor_green_200_steps, relative to the forced amplitude A / lam; v (analytically 0) <= 2e-6 max|u|.
    # measured on the MI355X: 6.6e-7 (64x64), 1.39e-6 (256x1024, U0 = 0.5), 1.44e-6 (1024x256, Ly = 4 pi): inside the expectation; v and p exactly 0
    k, A, nu, dt, n = 4, 1.0, 0.01, 0.01, 200
    lam = nu * (TWO_PI * k / Ly) ** 2 + drag
    s = solver(nx, ny, dt, 1.0, nu, Ly=Ly, drag=drag).kolmogorov_forcing(k, A)
    got, _ = run(s, np.full((nx, ny), U0), np.zeros((nx, ny)), n)
    ref = F.kolmogorov_laminar(nx, ny, n * dt, A, k, lam, Ly, U0)
    amp = A / lam * np.sin(TWO_PI * k * np.arange(ny) / ny)
    eu = np.linalg.norm(got[0][0] - ref[0]) / (np.linalg.norm(amp) * math.sqrt(nx))
    ev = np.abs(got[1]).max() / np.abs(got[0]).max()
    print('laminar Kolmogorov %dx%d Ly %.3g U0 %g drag %g: |u - exact| / |A / lam sin| %.2e, max|v| / max|u| %.2e, max|p| %.2e, lam t %.3g'
          % (nx, ny, Ly, U0, drag, eu, ev, np.abs(got[2]).max(), lam * n * dt))
    assert eu <= 2e-6 and ev <= 2e-6, (eu, ev)
    assert np.abs(ref[0] - U0).max() >= 0.1                      # the flow the force built is there to be compared


@pytest.mark.parametrize('nx,ny,Ly,U0,V0', [(64, 64, TWO_PI, 0.0, 0.0), (1024, 1024, TWO_PI, 0.5, -0.3), (64, 256, 2 * TWO_PI, 0.0, 0.0)])
def test_taylor_green_with_drag_200_steps(gpu_device, nx, ny, Ly, U0, V0):
    # the fluctuation decays by exp(-alpha t) on top of the viscous decay, the pressure by its square; the mean flow is not damped.
    # measured on the MI355X (u, v, p): 64x64 8.8e-8 8.4e-8 5.1e-8; 1024x1024 with the mean flow 2.4e-7 3.5e-7 1.0e-6; 64x256 8.6e-8 8.4e-8 9.9e-8
    dt, nu, rho, n, alpha = 0.01, 0.01, 1.0, 200, 0.4
    u0, v0, _ = O.taylor_green(nx, ny, 0.0, nu, rho, TWO_PI, Ly, U0, V0)
    got, _ = run(solver(nx, ny, dt, rho, nu, TWO_PI, Ly, drag=alpha), u0, v0, n)
    u, v, p = O.taylor_green(nx, ny, n * dt, nu, rho, TWO_PI, Ly, U0, V0)
    d = math.exp(-alpha * n * dt)
    ref = (U0 + (u - U0) * d, V0 + (v - V0) * d, p * d * d)
    errs = [rel_l2(g[0], r) for g, r in zip(got, ref)]
    print('Taylor-Green with drag %dx%d (U0, V0) = (%g, %g): rel-L2 u, v, p %s' % (nx, ny, U0, V0, ['%.2e' % e for e in errs]))
    assert max(errs) <= 2e-6, errs


# ---------------------------------------------------------------------------------------------------- 4. / 5. bitwise invariants
def test_shared_force_is_the_tiled_force_and_batch_members_are_the_single_runs(gpu_device):
    nx, ny, B = 128, 256, 3
    u0, v0 = O.random_ic(B, nx, ny, 8, seed=3, umax=1.5, mean=(0.2, 0.1))
    fx, fy = FC.random_forces(B, nx, ny, 17, TWO_PI, 2 * TWO_PI)
    s = solver(nx, ny, 0.01, 1.0, 0.005, Ly=2 * TWO_PI, drag=0.3)
    s.set_forcing(fx[:1], fy[:1])                                 # [1, nx, ny]: stored once
    _, shared = run(s, u0, v0, 12)
    s.set_forcing(np.repeat(fx[:1], B, axis=0), np.repeat(fy[:1], B, axis=0))
    assert s.ghat.shape[0] == B
    _, tiled = run(s, u0, v0, 12)
    assert torch.equal(shared.what, tiled.what)
    s.set_forcing(fx, fy)
    both, st = run(s, u0, v0, 12)
    again, st2 = run(s, u0, v0, 12)
    assert torch.equal(st.what, st2.what)
    for a, b in zip(both, again):
        assert np.array_equal(a, b)
    assert not torch.equal(st.what[1], shared.what[1])
    for k in range(B):
        s.set_forcing(fx[k], fy[k])
        one, st1 = run(s, u0[k:k + 1], v0[k:k + 1], 12)
        assert torch.equal(st1.what[0], st.what[k])
        for a, b in zip(one, both):
            assert np.array_equal(a[0], b[k])


def test_graph_replay_of_a_forced_run_is_bitwise_the_eager_loop(gpu_device):
    nx, ny = 64, 128
    u0, v0 = O.random_ic(2, nx, ny, 6, seed=5, umax=1.0)
    s = solver(nx, ny, 0.01, 1.0, 0.01, drag=0.2).kolmogorov_forcing(4, 2.0)
    eager = s.simulate(dev(u0), dev(v0), 12, save_every=3, use_graph=False)
    assert s.last_simulate_used_graph is False
    graphed = s.simulate(dev(u0), dev(v0), 12, save_every=3, use_graph=True)
    assert s.last_simulate_used_graph is True
    for a, b in zip(eager, graphed):
        assert a.shape == (5, 2, nx, ny) and torch.equal(a, b)
    stepped, _ = run(s, u0, v0, 12)
    assert np.array_equal(eager[0][-1].cpu().numpy().astype(np.float64), stepped[0])
    unforced = solver(nx, ny, 0.01, 1.0, 0.01).simulate(dev(u0), dev(v0), 12, save_every=3)
    assert rel_l2(eager[0][-1].cpu().numpy(), unforced[0][-1].cpu().numpy()) > 1e-2


# ---------------------------------------------------------------------------------------------------- 6. diagnostics
@pytest.mark.parametrize('case', [C.FULL_BAND[0], C.FULL_BAND[2]], ids=[C.case_id(C.FULL_BAND[0]), C.case_id(C.FULL_BAND[2])])
def test_diagnostics_against_the_oracle(gpu_device, case):
    nx, ny, B, Lx, Ly, mean = case
    u0, v0, dt = C.full_band_input(*case)
    S = FC.scheme(nx, ny, dt, Lx, Ly).kolmogorov_forcing(FC.KF, FC.AMP)
    s = solver(nx, ny, dt, C.RHO, C.NU, Lx, Ly, drag=FC.DRAG).kolmogorov_forcing(FC.KF, FC.AMP)
    w, _ = FC.oracle_run(S, u0, v0)
    _, st = run(s, u0, v0, C.NSTEPS)
    d = s.diagnostics(st)
    assert d._fields == ('energy', 'enstrophy', 'power_in')
    assert all(t.dtype == torch.float64 and tuple(t.shape) == (B,) for t in d)
    got = [t.cpu().numpy() for t in d]
    # (a) against the restatement's numbers of its own state: the state's error (BOUND_W, relative) twice in the quadratic E and Z, doubled
    # again for margin: 4 BOUND_W relative.  P = <f_s . u> is linear in the state: |dP| <= |f_s| |du| (Cauchy-Schwarz), so its error is
    # taken relative to rms(f_s) sqrt(2 E), same bound.  measured on the MI355X: E 2.2e-7, Z 1.1e-7, P 8.4e-8 (the larger of the two cases)
    ref = S.diag(w)
    fs = S.forcing_fields()
    pscale = np.sqrt((fs[0] ** 2 + fs[1] ** 2).mean()) * np.sqrt(2 * ref[0])
    ea = [np.abs(got[0] / ref[0] - 1).max(), np.abs(got[1] / ref[1] - 1).max(), (np.abs(got[2] - ref[2]) / pscale).max()]
    # (b) against the restatement's diag of the GPU state and force spectrum copied to the host: isolates the reduction.  Bound 1e-6
    # relative (a float32 1 / |k|^2 and float32 products would give 6e-8 each); the kernel forms them in float64.
    # measured on the MI355X: <= 3.3e-16 (E, Z, P)
    Sg = FC.scheme(nx, ny, dt, Lx, Ly)
    Sg.g = S.expand(state_c(s.ghat))
    own = Sg.diag(S.expand(state_c(st.what)))
    eb = [np.abs(g / r - 1).max() for g, r in zip(got, own)]
    print('diagnostics %dx%d B=%d: E %s Z %s P %s; vs oracle state (E, Z rel; P / (|f_s| |u|)) %s; vs oracle diag of the GPU state %s'
          % (nx, ny, B, got[0], got[1], got[2], ['%.2e' % e for e in ea], ['%.2e' % e for e in eb]))
    assert max(ea) <= 4 * C.BOUND_W, ea
    assert max(eb) <= 1e-6, eb
    assert np.abs(ref[2]).min() >= 1e-3 * pscale.max()           # the power input is there to be compared
    # without a force the power input is exactly 0.0, and energy and enstrophy do not change
    s.set_forcing(None)
    d0 = s.diagnostics(st)
    assert torch.equal(d0.power_in, torch.zeros(B, dtype=torch.float64, device='cuda'))
    assert torch.equal(d0.energy, d.energy) and torch.equal(d0.enstrophy, d.enstrophy)


def test_diagnostics_of_a_batch_member_are_the_single_state_s_and_repeat(gpu_device):
    nx, ny, B = 128, 256, 3
    u0, v0 = O.random_ic(B, nx, ny, 8, seed=3, umax=1.5, mean=(0.2, 0.1))
    fx, fy = FC.random_forces(B, nx, ny, 17, TWO_PI, 2 * TWO_PI)
    s = solver(nx, ny, 0.01, 1.0, 0.005, Ly=2 * TWO_PI, drag=0.3).set_forcing(fx, fy)
    _, st = run(s, u0, v0, 6)
    d, again = s.diagnostics(st), s.diagnostics(st)
    for a, b in zip(d, again):
        assert torch.equal(a, b)
    assert float(d.power_in.abs().min()) > 0 and float(d.energy.min()) > 0
    for k in range(B):
        s.set_forcing(fx[k], fy[k])
        _, st1 = run(s, u0[k:k + 1], v0[k:k + 1], 6)
        for a, b in zip(s.diagnostics(st1), d):
            assert torch.equal(a[0], b[k])


# ---------------------------------------------------------------------------------------------------- 7. residual of a forced trajectory
def test_residual_of_a_forced_trajectory_converges_to_the_force_minus_the_drag(gpu_device):
    # the set-up of test_gpu_pspec.py::test_residual_of_a_trajectory_is_first_order_in_dt under a Kolmogorov force (k = 4, A = 8) and drag
    # 2: the engine knows neither, so r_u -> f_sx - alpha (u - U0) (max ~ 12: it does not tend to zero), and what is left after
    # subtracting that is the (dt / 2) u_tt of its backward difference: it halves with dt.  On the CPU (tests/pspec_forced_oracle.py
    # frames through oracle/periodic.py: spectral_residual): ratios 2.016 and 2.011, max|r_u| 11.98 at both dt.
    # measured on the MI355X: 0.4662 -> 0.2312 (2.017) and 0.3648 -> 0.1813 (2.012); max|r_u| 11.98 at both dt
    n, nu, rho, t, A, alpha = 128, 0.01, 1.0, 0.1, 8.0, 2.0
    u0, v0 = O.random_ic(1, n, n, 4, seed=9, umax=4.0)
    out = {}
    for dt in (1e-2, 5e-3):
        s = solver(n, n, dt, rho, nu, drag=alpha).kolmogorov_forcing(4, A)
        U, V, P = s.simulate(dev(u0), dev(v0), int(round(t / dt)), save_every=1)
        r = s.residual_engine('spectral')(U[-1], V[-1], P[-1], U[-2], V[-2])
        fsx, fsy = s.forcing_fields()
        cu = r[0] - fsx + alpha * (U[-1] - U[-1].mean())
        cv = r[1] - fsy + alpha * (V[-1] - V[-1].mean())
        out[dt] = [float(x.abs().max()) for x in (cu, cv, r[0], r[1])]
    print('max|r_u - f_sx + alpha u\'|, same for v, max|r_u|, max|r_v| at dt = 1e-2 / 5e-3:', out)
    ru, rv = out[1e-2][0] / out[5e-3][0], out[1e-2][1] / out[5e-3][1]
    assert 1.8 <= ru <= 2.2 and 1.8 <= rv <= 2.2, (ru, rv)
    keep = out[1e-2][2] / out[5e-3][2]
    assert 1 / 1.2 <= keep <= 1.2 and out[5e-3][2] >= 10 * out[5e-3][0], out


# ---------------------------------------------------------------------------------------------------- 8. error codes
def test_error_codes(gpu_device):
    from nns import ops, _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_spec_ns_workspace(3, 64, 128, ctypes.byref(n)) == 0 and n.value > 0
    what = torch.zeros(3, 43, 64, 2, device='cuda')
    mean = torch.zeros(3, 2, device='cuda')
    g = torch.zeros(3, 43, 64, 2, device='cuda')
    work = torch.empty(n.value, dtype=torch.uint8, device='cuda')
    out = torch.empty(3, 3, dtype=torch.float64, device='cuda')
    p = lambda t: t.data_ptr()
    step = lambda gh, gb, drag, nx=64, wb=n.value: L.nns_spec_ns_step_forced_f32(p(what), p(mean), gh, gb, p(work), wb, 3, nx, 128, TWO_PI,
                                                                                 TWO_PI, 0.01, 0.0, drag, 1, None)
    assert step(p(g), 2, 0.0) == INVALID and b'gbatch' in L.nns_last_error()
    assert step(None, 1, 0.0) == INVALID
    assert step(p(g), 0, 0.0) == INVALID
    assert step(p(g), 3, -1.0) == INVALID and b'drag' in L.nns_last_error()
    assert step(p(g), 3, math.nan) == INVALID
    assert step(p(g), 3, 0.0, nx=96) == UNSUPPORTED
    assert step(p(g), 3, 0.0, wb=n.value - 1) == WORKSPACE
    assert L.nns_spec_ns_step_forced_f32(None, p(mean), None, 0, p(work), n.value, 3, 64, 128, TWO_PI, TWO_PI, 0.01, 0.0, 0.0, 1, None) == INVALID
    assert L.nns_spec_ns_step_forced_f32(p(what), p(mean), None, 0, p(work), n.value, 3, 64, 128, TWO_PI, TWO_PI, -0.01, 0.0, 0.0, 1, None) == INVALID
    assert step(p(g), 3, 0.5) == 0 and step(p(g), 1, 0.0) == 0 and step(None, 0, 0.5) == 0          # and the valid forms are accepted
    diag = lambda gh, gb, o, nx=64: L.nns_spec_ns_diag_f32(p(what), gh, gb, o, 3, nx, 128, TWO_PI, TWO_PI, None)
    assert diag(p(g), 3, None) == INVALID
    assert diag(p(g), 2, p(out)) == INVALID and diag(None, 1, p(out)) == INVALID and diag(p(g), 0, p(out)) == INVALID
    assert diag(None, 0, p(out), nx=96) == UNSUPPORTED
    assert diag(None, 0, p(out)) == 0 and diag(p(g), 1, p(out)) == 0
    torch.cuda.synchronize()
    # host: a per-grid force of the wrong batch, refused before any launch
    s = solver(64, 128, 0.01, 1.0, 0.0)
    z = torch.zeros(2, 64, 128, device='cuda')
    s.set_forcing(z, z)
    st = s.init(torch.zeros(3, 64, 128, device='cuda'), torch.zeros(3, 64, 128, device='cuda'))
    with pytest.raises(ValueError):
        s.step(st)
    with pytest.raises(ValueError):
        s.diagnostics(st)
    with pytest.raises(ValueError):
        s.simulate(torch.zeros(3, 64, 128, device='cuda'), torch.zeros(3, 64, 128, device='cuda'), 2)
    with pytest.raises(ValueError):
        ops.spec_ns_step_forced_(st.what, st.mean, s.ghat, st.work, 128, TWO_PI, TWO_PI, 0.01, 0.0, 0.0)
    with pytest.raises(TypeError):
        ops.spec_ns_step_forced_(st.what, st.mean, s.ghat.double(), st.work, 128, TWO_PI, TWO_PI, 0.01, 0.0, 0.0)
    with pytest.raises(ValueError):
        ops.spec_ns_diag(st.what, None, 64, TWO_PI, TWO_PI)
