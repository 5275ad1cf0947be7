"""GPU checks of the multigrid pressure solve (csrc/mg_kernels.hip through nns.ops.fd_poisson_mg_ and
NavierStokesSystem(pressure_solver='multigrid')) against the NumPy restatement tests/mg_oracle.py and the exact discrete solve."""
import ctypes

import numpy as np
import pytest
import torch

import mg_oracle as M
from conftest import rel_l2

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2


def dev(a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device='cuda')


def mg(p, C, dx, dy, **kw):
    from nns import ops
    info = ops.fd_poisson_mg_(p, C, dx, dy, **kw)
    torch.cuda.synchronize()
    return info.cpu().numpy()


def ring(a):
    a = np.asarray(a)
    return np.concatenate([a[..., 0, :], a[..., -1, :], a[..., :, 0], a[..., :, -1]], axis=-1)


@pytest.mark.parametrize('nx,ny', [(50, 50), (64, 50), (257, 257), (1024, 1024)])
def test_f64_follows_the_restatement_cycle_by_cycle(gpu_device, nx, ny):
    dx, dy = M.spacings(nx, ny)
    p, C = M.random_problem(nx, ny, seed=nx * 7 + ny)
    for k in (1, 2, 5):
        ref, rinfo, _ = M.solve_one(p, C, dx, dy, tol=0.0, max_cycles=k)
        pd = dev(p)
        info = mg(pd, dev(C), dx, dy, tol=0.0, max_cycles=k)
        got = pd.cpu().numpy()
        assert rel_l2(got, ref) <= 1e-11, (nx, ny, k, rel_l2(got, ref))
        assert int(info[0, 0]) == rinfo[0] == k
        assert abs(info[0, 1] - rinfo[1]) <= 1e-6 * rinfo[1]


@pytest.mark.parametrize('nx,ny', [(50, 50), (64, 50), (257, 257), (1024, 1024)])
def test_accuracy_against_the_exact_solve(gpu_device, nx, ny):
    dx, dy = M.spacings(nx, ny)
    p, C = M.random_problem(nx, ny, seed=11 + nx)
    ex = M.exact_solve(p, C, dx, dy)
    pd = dev(p)
    info = mg(pd, dev(C), dx, dy, tol=1e-10, max_cycles=30)
    assert rel_l2(pd.cpu().numpy(), ex) <= 1e-8 and info[0, 1] <= 1e-10 and 0 < info[0, 0] <= 14
    p32, C32 = p.astype(np.float32), C.astype(np.float32)
    ex32 = M.exact_solve(p32, C32, dx, dy)
    pd = dev(p32, np.float32)
    info = mg(pd, dev(C32, np.float32), dx, dy, tol=1e-6, max_cycles=30)
    err = rel_l2(pd.cpu().numpy(), ex32)
    assert err <= (1e-5 if nx * ny <= 64 * 64 else 5e-4), (nx, ny, err, info)
    assert info[0, 0] <= 12


def test_same_equation_as_the_reference_sor(gpu_device):
    from nns import ops
    n = 33
    dx, dy = M.spacings(n, n)
    p, C = M.random_problem(n, n, seed=5)
    C *= dx * dx * dy * dy                                                 # an O(1) solution: SOR's absolute tolerance is meaningful
    ps = dev(p)
    ops.fd_sor_(ps, dev(C), dx, dy, 1.8, 1e-13, 20000)
    pm = dev(p)
    mg(pm, dev(C), dx, dy, tol=1e-12, max_cycles=30)
    assert rel_l2(pm.cpu().numpy(), ps.cpu().numpy()) <= 1e-9


@pytest.mark.parametrize('nx,ny', [(50, 50), (257, 257)])
def test_boundary_ring_is_untouched(gpu_device, nx, ny):
    dx, dy = M.spacings(nx, ny)
    for dt in (np.float64, np.float32):
        p, C = M.random_problem(nx, ny, seed=2)
        p = p.astype(dt)
        pd = dev(p, dt)
        mg(pd, dev(C, dt), dx, dy, tol=1e-6)
        assert np.array_equal(ring(pd.cpu().numpy()), ring(p))


def _batch_problem(nx, ny):
    dx, dy = M.spacings(nx, ny)
    pa, Ca = M.random_problem(nx, ny, seed=21)
    pb = M.exact_solve(pa, Ca, dx, dy)                                     # already solved: stops at the rounding floor at once
    pc, Cc = np.full((nx, ny), 0.25), np.zeros((nx, ny))                 # zero residual: no cycle
    pdd, Cd = M.random_problem(nx, ny, seed=22)
    return np.stack([pa, pb, pc, pdd]), np.stack([Ca, Ca, Cc, Cd * 1e-3]), dx, dy


@pytest.mark.parametrize('nx,ny', [(50, 50), (257, 257)])
def test_batch_equals_single_grid_solves(gpu_device, nx, ny):
    P, Cs, dx, dy = _batch_problem(nx, ny)
    pb = dev(P)
    info = mg(pb, dev(Cs), dx, dy, tol=1e-8, max_cycles=30)
    got = pb.cpu().numpy()
    for b in range(4):
        ps = dev(P[b])
        inf1 = mg(ps, dev(Cs[b]), dx, dy, tol=1e-8, max_cycles=30)
        assert np.array_equal(got[b], ps.cpu().numpy()), b
        assert np.array_equal(info[b], inf1[0]), b
    cyc = info[:, 0].astype(int)
    assert cyc[2] == 0 and info[2, 1] == 0 and np.array_equal(got[2], P[2])
    assert cyc[0] >= 5 and cyc[1] <= 2 and cyc[3] >= 5
    assert len(set(cyc.tolist())) >= 3


def test_f32_stops_on_the_rounding_floor(gpu_device):
    nx = ny = 64
    dx, dy = M.spacings(nx, ny)
    p, C = M.random_problem(nx, ny, seed=8)
    pd = dev(p, np.float32)
    info = mg(pd, dev(C, np.float32), dx, dy, tol=1e-12, max_cycles=30)
    assert 2 <= info[0, 0] < 30 and info[0, 1] > 1e-12, info


@pytest.mark.parametrize('nx,ny', [(64, 64), (512, 512)])
def test_deterministic_and_hint_independent(gpu_device, nx, ny):
    dx, dy = M.spacings(nx, ny)
    P, Cs = M.random_problem(nx, ny, seed=9, B=3)
    outs = []
    for dt in (np.float64, np.float32):
        C = dev(Cs, dt)
        runs = []
        for hint in (None, None, 'one', 'many'):
            pd = dev(P, dt)
            h = None
            if hint == 'one':
                h = torch.tensor([[1.0, 0.0]] * 3, dtype=pd.dtype, device='cuda')
            elif hint == 'many':
                h = torch.tensor([[25.0, 0.0]] * 3, dtype=pd.dtype, device='cuda')
            info = mg(pd, C, dx, dy, tol=1e-6, max_cycles=30, hint=h)
            runs.append((pd.cpu().numpy(), info))
        for r in runs[1:]:
            assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
        outs.append(runs[0][1])
    assert all(o[:, 0].min() >= 1 for o in outs)


def test_argument_errors(gpu_device):
    from nns import _lib, ops
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    assert L.nns_fd_poisson_mg_workspace(1, 4, 64, 8, ctypes.byref(n)) == UNSUPPORTED
    assert L.nns_fd_poisson_mg_workspace(1, 1024, 64, 8, ctypes.byref(n)) == UNSUPPORTED          # coarsest level 128 x 8
    assert L.nns_fd_poisson_mg_workspace(0, 64, 64, 8, ctypes.byref(n)) == INVALID
    assert L.nns_fd_poisson_mg_workspace(1, 64, 64, 8, None) == INVALID
    assert L.nns_fd_poisson_mg_workspace(2, 64, 64, 8, ctypes.byref(n)) == 0 and n.value > 0
    p = torch.zeros(2, 64, 64, dtype=torch.float64, device='cuda')
    C = torch.zeros_like(p)
    info = torch.zeros(2, 2, dtype=torch.float64, device='cuda')
    work = torch.zeros(n.value, dtype=torch.uint8, device='cuda')
    args = lambda w, nx, dx, dy: (p.data_ptr(), C.data_ptr(), info.data_ptr(), w, 2, nx, 64, dx, dy, 1e-6, 3, 0, None)
    assert L.nns_fd_poisson_mg_f64(*args(None, 64, 0.03, 0.03)) == INVALID                          # missing workspace
    assert L.nns_fd_poisson_mg_f64(*args(work.data_ptr(), 64, 1.0, 0.3)) == UNSUPPORTED           # aspect ratio 3.3
    assert L.nns_fd_poisson_mg_f64(*args(work.data_ptr(), 4, 0.03, 0.03)) == UNSUPPORTED          # 4 nodes on an axis
    assert L.nns_fd_poisson_mg_f64(*args(work.data_ptr(), 64, 0.0, 0.03)) == INVALID
    with pytest.raises(_lib.NnsError):
        ops.fd_poisson_mg_(torch.zeros(64, 64, dtype=torch.float64, device='cuda'), torch.zeros(64, 64, dtype=torch.float64, device='cuda'), 1.0, 0.3)
    with pytest.raises(_lib.NnsError):
        ops.fd_poisson_mg_(torch.zeros(4, 64, dtype=torch.float64, device='cuda'), torch.zeros(4, 64, dtype=torch.float64, device='cuda'), 0.1, 0.1)


def _cavity(n, B=None, **kw):
    from src.chorin_fd.simulate import NavierStokesSystem
    from nns.boundary import DirichletBoundaryCondition as D, NeumannBoundaryCondition as N
    dx = dy = 2. / (n - 1)
    u_bc = [D(0, 'left', dx, dy), D(1, 'right', dx, dy), D(0, 'top', dx, dy), D(0, 'bottom', dx, dy)]
    v_bc = [D(0, 'left', dx, dy), D(0, 'right', dx, dy), D(0, 'top', dx, dy), D(0, 'bottom', dx, dy)]
    p_bc = [D(0, 'top', dx, dy), N(0, 'bottom', dx, dy), N(0, 'left', dx, dy), N(0, 'right', dx, dy)]
    shape = (n, n) if B is None else (B, n, n)
    rng = np.random.default_rng(4)
    u0 = 0.01 * rng.standard_normal(shape) if B is not None else np.zeros(shape)
    return NavierStokesSystem(u0, np.zeros(shape), np.zeros(shape), u_bc, v_bc, p_bc, nit=50, nx=n, ny=n, dt=1e-3, rho=1, nu=0.02, beta=1.25,
                              method='explicit', pressure_solver='multigrid', **kw), u0


def test_driver_cavity_multigrid(gpu_device):
    n = 64
    s, _ = _cavity(n, nt=20)
    assert s.pressure_solver == 'multigrid' and s.mg_tol == 1e-6 and s.mg_max_cycles == 30
    assert not s._fused_step_applies(torch.zeros(n, n, dtype=torch.float64, device='cuda'))
    u, v, p = s._init_variables()
    u1, v1 = u.clone(), v.clone()
    for step in range(20):
        un, vn, p = s.step(u, v, u1, v1, p)
        (cycles, ratio), = s.sor_info()
        assert ratio <= 1e-6 and 1 <= cycles <= 30, (step, cycles, ratio)
        u1, v1, u, v = u, v, un, vn
    for t in (u, v, p):
        assert bool(torch.isfinite(t).all())
    assert float(p.abs().max()) > 0
    us, vs, ps = s.simulate_device()
    assert all(bool(torch.isfinite(t).all()) for t in (us, vs, ps))
    with pytest.raises(ValueError):
        s.simulate_device(use_graph=True)


def test_driver_ensemble_members_equal_single_runs(gpu_device):
    n = 64
    s, u0 = _cavity(n, B=2, nt=10)
    us, vs, ps = s.simulate()
    for b in range(2):
        s1, _ = _cavity(n, nt=10)
        s1.u_ic = u0[b]
        u1, v1, p1 = s1.simulate()
        assert np.array_equal(us[:, b], u1) and np.array_equal(vs[:, b], v1) and np.array_equal(ps[:, b], p1), b
