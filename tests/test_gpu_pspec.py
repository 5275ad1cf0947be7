"""GPU checks of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip through nns.periodic.PeriodicSolver) against the analytic
Taylor-Green vortex, the float64 restatement tests/pspec_oracle.py and the spectral residual engine."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_oracle as O
from conftest import rel_l2

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


def host(ts):
    return [t.cpu().numpy().astype(np.float64) for t in ts]


def solver(nx, ny, dt, rho, nu, Lx=TWO_PI, Ly=TWO_PI):
    from nns.periodic import PeriodicSolver
    return PeriodicSolver(nx, ny, dt, rho, nu, Lx=Lx, Ly=Ly)


def run(s, u0, v0, nsteps):
    st = s.init(dev(u0), dev(v0))
    s.step(st, nsteps)
    out = host(s.fields(st))
    return out, st


def test_init_and_fields_against_the_oracle(gpu_device):
    nx, ny, Lx, Ly, rho = 128, 64, 3.0, 1.5, 1.7
    # neither divergence-free nor band-limited: independent random u and v spectra over every wavenumber, amplitude 1 / (1 + |m|^2)
    rng = np.random.default_rng(7)
    mx, my = np.fft.fftfreq(nx) * nx, np.arange(ny // 2 + 1)
    amp = 1.0 / (1.0 + mx[:, None] ** 2 + my[None, :] ** 2)
    spec = (rng.standard_normal((2, 3, nx, ny // 2 + 1)) + 1j * rng.standard_normal((2, 3, nx, ny // 2 + 1))) * amp
    u, v = np.fft.irfft2(spec, s=(nx, ny)).astype(np.float32) * 100
    S = O.Scheme(nx, ny, 0.01, rho, 0.0, Lx=Lx, Ly=Ly)
    w, mean = S.init(u, v)
    ref = S.fields(w, mean)
    s = solver(nx, ny, 0.01, rho, 0.0, Lx, Ly)
    st = s.init(dev(u), dev(v))
    got = host(s.fields(st))
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    print('init/fields rel-L2 u, v, p:', ['%.2e' % e for e in errs])
    # float32 transforms, measured on the MI355X on these fields: u, v 1.7e-7, p 3.5e-7 (a product of derivatives, one more transform
    # pair).  On white noise, where the highest wavenumbers dominate p, u and v measured 1.9e-7 and p 9.7e-6: hence the smoother fields
    assert errs[0] <= 1e-6 and errs[1] <= 1e-6 and errs[2] <= 3e-6, errs
    # divergence-free and masked to the float32 rounding of the output: |div| relative to k_max max|u|, spectrum outside the 2/3 band
    kmax = max(np.pi * nx / Lx, np.pi * ny / Ly)
    div = S.divergence(got[0], got[1])
    assert np.abs(div).max() <= 1e-6 * kmax * np.abs(got[0]).max(), np.abs(div).max()
    outside = 1 - S.M
    outside[0, 0] = 0
    for g in got[:2]:
        gh = np.fft.rfft2(g)
        assert np.linalg.norm(gh * outside) <= 1e-6 * np.linalg.norm(gh)
    what = st.what.cpu().numpy().astype(np.float64)
    ref_w = S.compact(w)
    assert np.linalg.norm(what[..., 0] + 1j * what[..., 1] - ref_w) <= 1e-6 * np.linalg.norm(ref_w)
    assert np.abs(st.mean.cpu().numpy() - mean).max() <= 1e-6


TG = [(64, 64, TWO_PI, TWO_PI), (256, 256, TWO_PI, TWO_PI), (1024, 1024, TWO_PI, TWO_PI), (64, 256, TWO_PI, 2 * TWO_PI)]


@pytest.mark.parametrize('nx,ny,Lx,Ly', TG)
@pytest.mark.parametrize('U0,V0', [(0.0, 0.0), (0.5, -0.3)])
def test_taylor_green_200_steps(gpu_device, nx, ny, Lx, Ly, U0, V0):
    dt, nu, rho, n = 0.01, 0.01, 1.0, 200
    u0, v0, _ = O.taylor_green(nx, ny, 0.0, nu, rho, Lx, Ly, U0, V0)
    got, _ = run(solver(nx, ny, dt, rho, nu, Lx, Ly), u0, v0, n)
    ref = O.taylor_green(nx, ny, n * dt, nu, rho, Lx, Ly, U0, V0)
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    print('Taylor-Green %dx%d (U0, V0) = (%g, %g): rel-L2 u, v, p %s' % (nx, ny, U0, V0, ['%.2e' % e for e in errs]))
    # float32 state, 200 steps: the decay is applied as w + expm1(L dt / 2) w (no systematic rounding of E); the mean-flow case
    # advects through the nonlinear path.  Measured on the MI355X over all 8 cases: u, v <= 3.6e-7, p <= 6.5e-7 -- 3x margin
    assert max(errs) <= 2e-6, errs


def test_random_band_limited_ic_against_the_oracle(gpu_device):
    nx, ny, dt, rho, nu, n = 128, 128, 0.005, 1.0, 0.01, 50
    u0, v0 = O.random_ic(4, nx, ny, 8, seed=11, umax=2.0)
    u0, v0 = u0.astype(np.float32), v0.astype(np.float32)
    ref = O.Scheme(nx, ny, dt, rho, nu).simulate(u0, v0, n, save_every=n)
    got, _ = run(solver(nx, ny, dt, rho, nu), u0, v0, n)
    errs = [rel_l2(g, r[-1]) for g, r in zip(got, ref)]
    print('random |m| <= 8, B = 4, 50 steps: rel-L2 u, v, p vs float64 oracle %s' % (['%.2e' % e for e in errs],))
    # measured on the MI355X: 5.2e-7, 4.6e-7, 6.9e-7 (float32 rounding; the scheme is the oracle's) -- bound with 7x margin
    assert max(errs) <= 5e-6, errs


def test_batch_members_are_bitwise_the_single_runs_and_runs_repeat(gpu_device):
    nx, ny = 128, 256
    u0, v0 = O.random_ic(3, nx, ny, 8, seed=3, umax=1.5, mean=(0.2, 0.1))
    s = solver(nx, ny, 0.01, 1.0, 0.005, Lx=TWO_PI, Ly=2 * TWO_PI)
    both, st = run(s, u0, v0, 12)
    again, st2 = run(s, u0, v0, 12)
    assert torch.equal(st.what, st2.what)
    for a, b in zip(both, again):
        assert np.array_equal(a, b)
    for k in range(3):
        one, st1 = run(s, u0[k:k + 1], v0[k:k + 1], 12)
        assert torch.equal(st1.what[0], st.what[k])
        for a, b in zip(one, both):
            assert np.array_equal(a[0], b[k])


def test_graph_replay_is_bitwise_the_eager_loop(gpu_device):
    nx, ny = 64, 128
    u0, v0 = O.random_ic(2, nx, ny, 6, seed=5, umax=1.0)
    s = solver(nx, ny, 0.01, 1.0, 0.01)
    eager = s.simulate(dev(u0), dev(v0), 12, save_every=3, use_graph=False)
    assert s.last_simulate_used_graph is False
    graphed = s.simulate(dev(u0), dev(v0), 12, save_every=3, use_graph=True)
    assert s.last_simulate_used_graph is True
    for a, b in zip(eager, graphed):
        assert a.shape == (5, 2, nx, ny) and torch.equal(a, b)
    stepped, _ = run(s, u0, v0, 12)                      # the frames are the step / fields path's
    assert np.array_equal(eager[0][-1].cpu().numpy().astype(np.float64), stepped[0])


def test_residual_of_a_trajectory_is_first_order_in_dt(gpu_device):
    # |m| <= 4 initial condition: the products live in |m| <= 8, far inside the 2/3 band, so the residual measures the time
    # discretisation of its own backward difference, (dt / 2) u_tt: halving dt halves it
    n, nu, rho, t = 128, 0.01, 1.0, 0.1
    u0, v0 = O.random_ic(1, n, n, 4, seed=9, umax=4.0)
    out = {}
    for dt in (1e-2, 5e-3):
        s = solver(n, n, dt, rho, nu)
        U, V, P = s.simulate(dev(u0), dev(v0), int(round(t / dt)), save_every=1)
        eng = s.residual_engine('spectral')
        r = eng(U[-1], V[-1], P[-1], U[-2], V[-2])
        out[dt] = [float(x.abs().max()) for x in r]
        out[dt].append(float(U[-1].abs().max()))
    print('max|r_u|, max|r_v|, max|r_div|, max|u| at dt = 1e-2 / 5e-3:', out)
    ru = out[1e-2][0] / out[5e-3][0]
    rv = out[1e-2][1] / out[5e-3][1]
    assert 1.8 <= ru <= 2.2 and 1.8 <= rv <= 2.2, (ru, rv)
    # measured on the MI355X: ratios 2.00 and 2.01 (max|r_u| 0.50 -> 0.25); max|r_div| 2.6e-5 / 2.8e-5 at max|u| = 3.5: float32
    # rounding of spectral derivatives of the frames (the solver's own output is divergence-free by construction); bound 5x above that
    for dt in out:
        assert out[dt][2] <= 1e-5 * out[dt][3] * 4, out


def test_error_codes(gpu_device):
    from nns import ops, _lib
    with pytest.raises(_lib.NnsError, match=r'\(-2\).*power of two'):
        ops.spec_ns_workspace(1, 96, 64)
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_spec_ns_workspace(1, 64, 96, ctypes.byref(n)) == UNSUPPORTED and b'power of two' in L.nns_last_error()
    assert L.nns_spec_ns_workspace(0, 64, 64, ctypes.byref(n)) == INVALID
    assert L.nns_spec_ns_workspace(2, 64, 128, ctypes.byref(n)) == 0 and n.value > 0
    u = torch.zeros(2, 64, 128, device='cuda')
    what = torch.empty(2, 43, 64, 2, device='cuda')
    mean = torch.empty(2, 2, device='cuda')
    work = torch.empty(n.value, dtype=torch.uint8, device='cuda')
    p = lambda t: t.data_ptr()
    assert L.nns_spec_ns_init_f32(p(u), p(u), p(what), p(mean), p(work), n.value - 1, 2, 64, 128, TWO_PI, TWO_PI, None) == WORKSPACE
    assert L.nns_spec_ns_init_f32(p(u), None, p(what), p(mean), p(work), n.value, 2, 64, 128, TWO_PI, TWO_PI, None) == INVALID
    assert L.nns_spec_ns_step_f32(p(what), p(mean), p(work), n.value, 2, 96, 128, TWO_PI, TWO_PI, 0.01, 0.0, 1, None) == UNSUPPORTED
    assert L.nns_spec_ns_step_f32(p(what), p(mean), p(work), n.value, 2, 64, 128, TWO_PI, TWO_PI, -0.01, 0.0, 1, None) == INVALID
    assert L.nns_spec_ns_fields_f32(p(what), p(mean), p(u), p(u), p(u), p(work), 16, 2, 64, 128, TWO_PI, TWO_PI, 1.0, None) == WORKSPACE
    s = solver(64, 128, 0.01, 1.0, 0.0)
    with pytest.raises(TypeError):
        s.init(u.double(), u.double())
    with pytest.raises(ValueError):
        s.step(solver(64, 64, 0.01, 1.0, 0.0).init(torch.zeros(1, 64, 64, device='cuda'), torch.zeros(1, 64, 64, device='cuda')))
