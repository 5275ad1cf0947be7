"""GPU checks of the multigrid pressure solve (csrc/mg_kernels.hip) where its kernels can go wrong and tests/test_gpu_multigrid.py does not
look: every launch path in both types (single level, all in LDS, chip-wide + LDS tail), the two LDS-maximal launches and the first sizes past
them, non-square boxes, a cell aspect of exactly 2, aspect drift on non-nested levels, batches over 256 and over 1024 grids, non-finite
data, non-default streams and the cavity driver.  The reference is the float64 restatement tests/mg_oracle.py; the cases and bounds are in
tests/mg_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import mg_cases as K
import mg_oracle as M
from conftest import rel_l2

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
CASES = [c for c, _ in K.CASES]
IDS = [K.case_id(c) for c in CASES]
SINGLE = [c for c in CASES if K.path(c[0], c[1], 8) == 'single']


def dev(a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device='cuda')


def mg(p, C, dx, dy, **kw):
    from nns import ops
    info = ops.fd_poisson_mg_(p, C, dx, dy, **kw)
    torch.cuda.synchronize()
    return info.cpu().numpy()


def info_matches(got, ref):
    """Equal cycle counts; ratios equal to 1e-6 relative, or both at the float64 rounding floor."""
    if int(got[0]) != ref[0]:
        return False
    return abs(got[1] - ref[1]) <= 1e-6 * ref[1] if ref[1] > 1e-9 else got[1] <= 1e-10


# ---------------------------------------------------------------------------------------------------- a. the launch paths
def test_workspace_pins_the_launch_path(gpu_device):
    """The workspace size is a strictly increasing function of the split, so the size the library reports fixes its tail level."""
    from nns import ops
    seen = set()
    for nx, ny, B, _, _ in CASES:
        nlev = len(M.levels(nx, ny))
        for elem in (4, 8):
            for b in sorted({1, B, 300, 1100}):
                got = ops.fd_poisson_mg_workspace(b, nx, ny, elem)
                assert got == M.workspace_bytes(b, nx, ny, elem), (nx, ny, b, elem, got)
                assert [t for t in range(nlev) if M.workspace_bytes(b, nx, ny, elem, tail=t) == got] == [M.tail_level(nx, ny, elem)]
            seen.add((K.path(nx, ny, elem), elem))
    assert seen == {(p, e) for p in ('single', 'lds', 'mixed') for e in (4, 8)}
    squares = {c[0] for c in CASES if c[0] == c[1]}
    for n, t32, t64 in ((84, 0, 0), (85, 0, 1), (119, 0, 1), (120, 1, 1), (200, 1, 2)):
        assert n in squares and (M.tail_level(n, n, 4), M.tail_level(n, n, 8)) == (t32, t64)


# ---------------------------------------------------------------------------------------------------- b. cycle by cycle
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f64_follows_the_restatement_cycle_by_cycle(gpu_device, case):
    nx, ny, B, dx, dy = case
    P, Cs = K.problem(case)
    ks = (1,) if K.path(nx, ny, 8) == 'single' else K.cycles_checked(nx, ny)     # one cycle of the exact solve reaches the rounding floor
    for k in ks:
        pd = dev(P)
        info = mg(pd, dev(Cs), dx, dy, tol=0.0, max_cycles=k)
        got = pd.cpu().numpy()
        for b in range(B):
            ref, rinfo, _ = M.solve_one(P[b], Cs[b], dx, dy, tol=0.0, max_cycles=k)
            err = rel_l2(got[b], ref)
            assert err <= K.BOUND_F64, (case, k, b, err)
            assert rinfo[0] == k and info_matches(info[b], rinfo), (case, k, b, info[b], rinfo)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f32_follows_the_restatement_cycle_by_cycle(gpu_device, case):
    """float32 against the float64 restatement started from the same float32-rounded p and C."""
    nx, ny, B, dx, dy = case
    P, Cs = K.problem(case)
    P32, C32 = P.astype(np.float32), Cs.astype(np.float32)
    path = K.path(nx, ny, 4)
    for k in ((1,) if path == 'single' else (1, 2)):
        bound = K.BOUND_F32[path, k]
        pd = dev(P32, np.float32)
        info = mg(pd, dev(C32, np.float32), dx, dy, tol=0.0, max_cycles=k)
        got = pd.cpu().numpy()
        errs = []
        for b in range(B):
            ref, rinfo, _ = M.solve_one(P32[b].astype(np.float64), C32[b].astype(np.float64), dx, dy, tol=0.0, max_cycles=k)
            errs.append(rel_l2(got[b], ref))
            assert int(info[b, 0]) == rinfo[0] == k, (case, k, b, info[b], rinfo)
            if path != 'single':                                            # a single-level ratio is float32 rounding noise
                assert abs(info[b, 1] - rinfo[1]) <= 1e-3 * rinfo[1], (case, k, b, info[b], rinfo)
        print('f32 %s path %s tail %d k=%d: rel-L2 %.2e (bound %.1e)' % (K.case_id(case), path, M.tail_level(nx, ny, 4), k, max(errs), bound))
        assert max(errs) <= bound, (case, k, errs)


@pytest.mark.parametrize('case', SINGLE, ids=[K.case_id(c) for c in SINGLE])
def test_single_level_is_the_exact_solve(gpu_device, case):
    nx, ny, B, dx, dy = case
    P, Cs = K.problem(case)
    ex = np.stack([M.exact_solve(P[b], Cs[b], dx, dy) for b in range(B)])
    for cycles in (1, 30):
        pd = dev(P)
        info = mg(pd, dev(Cs), dx, dy, tol=0.0, max_cycles=cycles)
        got = pd.cpu().numpy()
        for b in range(B):
            assert rel_l2(got[b], ex[b]) <= 1e-12, (case, cycles, b, rel_l2(got[b], ex[b]))
            assert info[b, 1] <= 1e-12, (case, cycles, info[b])
            if cycles == 1:
                assert int(info[b, 0]) == 1
            else:                                                           # the stagnation rule ends it at the rounding floor
                assert 2 <= int(info[b, 0]) <= 6, (case, info[b])


# ---------------------------------------------------------------------------------------------------- c. refusals
@pytest.mark.parametrize('nx,ny,dx,dy,refused', K.SHAPE_CHECKS)
def test_refused_exactly_when_the_restatement_refuses(gpu_device, nx, ny, dx, dy, refused):
    from nns import _lib
    L = _lib.lib()
    try:
        M.hierarchy(nx, ny, dx, dy)
        oracle_refuses = False
    except M.UnsupportedGrid:
        oracle_refuses = True
    assert oracle_refuses == refused
    n = ctypes.c_size_t(0)
    rc = L.nns_fd_poisson_mg_workspace(1, nx, ny, 8, ctypes.byref(n))
    work = torch.zeros(max(n.value if rc == 0 else 0, 256), dtype=torch.uint8, device='cuda')
    p = torch.zeros(nx, ny, dtype=torch.float64, device='cuda')
    C = torch.zeros_like(p)
    info = torch.full((1, 2), -7.0, dtype=torch.float64, device='cuda')
    rc = L.nns_fd_poisson_mg_f64(p.data_ptr(), C.data_ptr(), info.data_ptr(), work.data_ptr(), 1, nx, ny, dx, dy, 1e-6, 1, 0, None)
    torch.cuda.synchronize()
    assert rc == (UNSUPPORTED if refused else 0), (nx, ny, dx / dy, rc)
    assert info.cpu().tolist() == ([[-7.0, -7.0]] if refused else [[0.0, 0.0]])          # a zero problem: no cycle, (0, 0)


# ---------------------------------------------------------------------------------------------------- d. large batches
def mixed_batch(nx, ny, B, seed):
    """Members b % 4: 0 random, 1 already solved, 2 zero residual, 3 far from solved (a large rough interior)."""
    dx, dy = M.spacings(nx, ny)
    P, Cs = M.random_problem(nx, ny, seed=seed, B=B)
    rng = np.random.default_rng(seed + 1)
    kind = np.arange(B) % 4
    for b in np.nonzero(kind == 1)[0]:
        P[b] = M.exact_solve(P[b], Cs[b], dx, dy)
    P[kind == 2] = 0.25
    Cs[kind == 2] = 0.0
    P[kind == 3, 1:-1, 1:-1] = 1e3 * rng.standard_normal((int((kind == 3).sum()), nx - 2, ny - 2))
    return P, Cs, dx, dy, kind


def sampled_members(B):
    """The first two, both sides of every edge between blocks of 256 grids, the last."""
    s = {0, 1, B - 1}
    for e in range(256, B, 256):
        s |= {e - 1, e}
    return sorted(s)


@pytest.mark.parametrize('nx,ny,B,dtype', K.BATCH_CASES, ids=['%dx%dxB%d_%s' % c for c in K.BATCH_CASES])
def test_large_batch_members_equal_single_solves(gpu_device, nx, ny, B, dtype):
    t = np.dtype(dtype).type
    P, Cs, dx, dy, kind = mixed_batch(nx, ny, B, seed=B + nx)
    pb = dev(P, t)
    info = mg(pb, dev(Cs, t), dx, dy, tol=1e-6, max_cycles=30)
    got = pb.cpu().numpy()
    for b in sampled_members(B):
        ps = dev(P[b], t)
        inf1 = mg(ps, dev(Cs[b], t), dx, dy, tol=1e-6, max_cycles=30)
        assert np.array_equal(got[b], ps.cpu().numpy()), b
        assert np.array_equal(info[b], inf1[0]), (b, info[b], inf1[0])
    cyc = info[:, 0].astype(int)
    z = kind == 2
    assert (cyc[z] == 0).all() and (info[z, 1] == 0).all() and np.array_equal(got[z], P[z].astype(t))
    assert (cyc[~z] >= 1).all() and np.isfinite(info[:, 1]).all()
    assert cyc[kind == 1].max() < cyc[kind == 0].min() and len(set(cyc.tolist())) >= 3, sorted(set(cyc.tolist()))


# ---------------------------------------------------------------------------------------------------- e. non-finite data
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('n', [64, 129])                # tail 0 and tail 1 in both types
def test_non_finite_members_report_nan(gpu_device, n, dtype):
    """A NaN or Inf in C or p is never reported as a zero residual ((0, 0), 'already solved'): such a member reports (0, NaN), runs no cycle
    and keeps p; the finite members of the batch are unaffected."""
    t = np.dtype(dtype).type
    dx, dy = M.spacings(n, n)
    P, Cs = M.random_problem(n, n, seed=31, B=7)
    Cs[1, n // 2, n // 3] = np.nan
    Cs[3, 5, 7] = np.inf
    P[4, 0, n // 2] = np.nan                                               # the boundary ring
    P[5, n // 3, n // 2] = -np.inf                                         # the interior
    bad, good = [1, 3, 4, 5], [0, 2, 6]
    pb = dev(P, t)
    info = mg(pb, dev(Cs, t), dx, dy, tol=1e-6, max_cycles=30)
    got = pb.cpu().numpy()
    for b in good:
        ps = dev(P[b], t)
        inf1 = mg(ps, dev(Cs[b], t), dx, dy, tol=1e-6, max_cycles=30)
        assert np.array_equal(got[b], ps.cpu().numpy()) and np.array_equal(info[b], inf1[0]), b
        assert int(info[b, 0]) >= 1 and np.isfinite(info[b, 1]), (b, info[b])
    for b in bad:
        assert int(info[b, 0]) == 0 and np.isnan(info[b, 1]), (b, info[b])
        assert np.array_equal(got[b], P[b].astype(t), equal_nan=True), b
        _, rinfo, _ = M.solve_one(P[b], Cs[b], dx, dy)
        assert rinfo[0] == 0 and np.isnan(rinfo[1])


# ---------------------------------------------------------------------------------------------------- f. streams
@pytest.mark.parametrize('n', [64, 129])                # tail 0, tail 1
def test_non_default_stream_is_bitwise_the_default(gpu_device, n):
    from nns import ops
    dx, dy = M.spacings(n, n)
    P, Cs = M.random_problem(n, n, seed=41, B=3)
    pa = dev(P)
    ia = mg(pa, dev(Cs), dx, dy, tol=1e-8)
    src_p, src_C = dev(P), dev(Cs)
    pb, Cb = torch.zeros_like(src_p), torch.zeros_like(src_C)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the side stream holds its inputs back: a launch on any other stream would solve a zero problem
        torch.cuda._sleep(20_000_000)
        pb.copy_(src_p)
        Cb.copy_(src_C)
        ib = ops.fd_poisson_mg_(pb, Cb, dx, dy, tol=1e-8)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(pb.cpu().numpy(), pa.cpu().numpy()) and np.array_equal(ib.cpu().numpy(), ia)
    assert (ia[:, 0] >= 5).all()


# ---------------------------------------------------------------------------------------------------- g. the cavity driver
@pytest.mark.parametrize('n', [50, 129])                # tail 0, tail 1
def test_driver_cavity_follows_the_composed_oracle(gpu_device, n):
    """NavierStokesSystem(method='explicit', pressure_solver='multigrid') against the same steps composed from oracle/chorin_fd.py's predictor,
    boundary conditions, pressure_rhs and correction, with mg_oracle.solve as the pressure solve."""
    from nns.chorin_fd import NavierStokesSystem
    from oracle import chorin_fd as OC
    from oracle.boundary import apply_bc_list, cavity_bcs
    dt, nu, rho, steps = 1e-3, 0.02, 1.0, 10
    dx = dy = 2.0 / (n - 1)
    u_bc, v_bc, p_bc = cavity_bcs(dx, dy)
    z = np.zeros((n, n))
    s = NavierStokesSystem(z.copy(), z.copy(), z.copy(), u_bc, v_bc, p_bc, nt=steps, nit=50, nx=n, ny=n, dt=dt, rho=rho, nu=nu, beta=1.25,
                           method='explicit', pressure_solver='multigrid')
    u, v, p = s._init_variables()
    u1, v1 = u.clone(), v.clone()
    ou, ov, op = (apply_bc_list(z.copy(), bc) for bc in (u_bc, v_bc, p_bc))
    ou1, ov1 = ou.copy(), ov.copy()
    for step in range(steps):
        un, vn, p = s.step(u, v, u1, v1, p)
        (cycles, ratio), = s.sor_info()
        u1, v1, u, v = u, v, un, vn
        ui, vi = OC.explicit_predictor(ou, ov, ou1, ov1, dt, dx, dy, nu)
        apply_bc_list(ui, u_bc)
        apply_bc_list(vi, v_bc)
        op, rinfo = M.solve(op, OC.pressure_rhs(ui, vi, dt, dx, dy, rho), dx, dy, tol=s.mg_tol, max_cycles=s.mg_max_cycles)
        apply_bc_list(op, p_bc)
        oun, ovn = OC.correction(ui, vi, op, dt, dx, dy)
        ou1, ov1, ou, ov = ou, ov, oun, ovn
        errs = [rel_l2(g.cpu().numpy(), r) for g, r in ((u, ou), (v, ov), (p, op))]
        assert cycles == int(rinfo[0, 0]) and 1 <= cycles < 30 and ratio <= 1e-6, (step, cycles, ratio, rinfo)
        assert max(errs) <= 1e-9, (step, errs)
    assert float(np.abs(op).max()) > 0
