"""GPU checks of the shell spectra and spectral transfers of the pseudo-spectral periodic solver (csrc/pspec_kernels.hip: nns_spec_ns_shells,
nns_spec_ns_spectrum_f32, nns_spec_ns_transfer_f32, through nns.periodic.PeriodicSolver.spectrum / transfer / energy_budget) against the float64
restatement tests/pspec_spectrum_oracle.py applied to the state the GPU holds, and of their bitwise contracts."""
import ctypes

import numpy as np
import pytest
import torch

import pspec_cases as C
import pspec_forced_cases as FC
import pspec_scalar_cases as SC
import pspec_spectrum_cases as PC
import pspec_spectrum_oracle as PO

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi
IDS = [C.case_id(c) for c in PC.CASES]


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device='cuda')          # a copy: the shared inputs are read-only


def state_c(t):
    w = t.cpu().numpy().astype(np.float64)
    return w[..., 0] + 1j * w[..., 1]


def solver(nx, ny, dt, Lx=TWO_PI, Ly=TWO_PI, forced=True, kappa=SC.KAPPA):
    from nns.periodic import PeriodicSolver
    s = PeriodicSolver(nx, ny, dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=FC.DRAG if forced else 0.0, kappa=kappa, scalar_gradient=SC.GRAD)
    return s.kolmogorov_forcing(FC.KF, FC.AMP) if forced else s


_RUNS = {}


def case_run(case):
    """(solver, state, scheme, w, t): a case after NSTEPS forced steps with its scalar, and the restatement's scheme holding the GPU's own
    force spectrum with the GPU's state in rfft2 layout (float64 copies of the float32 numbers).  Run once; the state is never stepped."""
    if case not in _RUNS:
        nx, ny, B, Lx, Ly, _ = case
        S, u0, v0, th0 = PC.reference(case)[:4]
        s = solver(nx, ny, S.dt, Lx, Ly)
        st = s.init(dev(u0), dev(v0), dev(th0))
        s.step(st, PC.NSTEPS)
        T = SC.scheme(nx, ny, S.dt, Lx, Ly)
        T.g = T.expand(state_c(s.ghat))
        _RUNS[case] = (s, st, T, T.expand(state_c(st.what)), T.expand(state_c(st.that)))
    return _RUNS[case]


def npy(x):
    return x.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 1. spectrum
@pytest.mark.parametrize('case', PC.CASES, ids=IDS)
def test_spectrum_against_the_oracle_of_the_same_state(gpu_device, case):
    # both sides sum the same float32 spectrum in float64: only the order differs (PC.BOUND_SPECTRUM: <= ~7000 terms per shell at 2^-53 each)
    # measured on the MI355X over the five cases: per shell E, Z, V <= 1.0e-15 relative, F exact, row sums against the diagnostics <= 4.4e-16
    nx, ny, B, Lx, Ly, _ = case
    s, st, T, w, t = case_run(case)
    ref = PO.spectrum(T, w, t)
    k, dk = s.shells()
    ok, odk, S = PO.shells(nx, ny, Lx, Ly)
    assert k.dtype == np.float64 and k.shape == (S,) and dk == odk and np.array_equal(k, ok)
    sp = s.spectrum(st)
    assert sp._fields == ('k', 'energy', 'enstrophy', 'injection', 'variance') and np.array_equal(sp.k, k)
    assert all(x.dtype == torch.float64 and tuple(x.shape) == (B, S) and x.is_cuda for x in sp[1:])
    errs = {}
    for name, got in (('E', sp.energy), ('Z', sp.enstrophy), ('V', sp.variance)):
        got, r = npy(got), ref[name]
        live = r > 0
        assert (got[~live] == 0).all() and live[:, -1].all() and not live[:, 0].any()          # shell 0 is empty, the corner's shell is the last
        errs[name] = np.abs(got[live] / r[live] - 1).max()
    gF, live = npy(sp.injection), ref['A_F'] > 0
    assert (gF[~live] == 0).all() and live.any()
    errs['F'] = (np.abs(gF - ref['F'])[live] / ref['A_F'][live]).max()
    d, sd = s.diagnostics(st), s.scalar_diagnostics(st)
    sums = [np.abs(npy(a.sum(-1)) / npy(b) - 1).max() for a, b in ((sp.energy, d.energy), (sp.enstrophy, d.enstrophy), (sp.injection, d.power_in),
                                                                  (sp.variance, sd.variance))]
    print('spectrum %dx%d B=%d S=%d: per shell E %.1e Z %.1e V %.1e (relative), F %.1e of its scale; row sums against the diagnostics %s'
          % (nx, ny, B, S, errs['E'], errs['Z'], errs['V'], errs['F'], ['%.1e' % x for x in sums]))
    assert max(errs.values()) <= PC.BOUND_SPECTRUM, errs
    assert max(sums) <= PC.BOUND_SPECTRUM, sums


# ---------------------------------------------------------------------------------------------------- 2. single modes
@pytest.mark.parametrize('shape', [(64, 64), (1024, 64)], ids=['64x64', '1024x64'])
def test_a_single_mode_lands_in_the_shell_the_oracle_names(gpu_device, shape):
    nx, ny = shape
    Lx, Ly = (TWO_PI, TWO_PI) if nx == ny else (3.0, TWO_PI)
    s = solver(nx, ny, 1e-3, Lx, Ly, forced=False, kappa=None)
    T = FC.scheme(nx, ny, 1e-3, Lx, Ly)
    kmx, my1 = (nx - 1) // 3, s.my1
    # (m_x, j) per grid: m_x < 0, the j = 0 line (with its conjugate partner), the band's two corners
    modes = [(-5, 3), (7, 0), (kmx, my1 - 1), (-kmx, my1 - 1)]
    z = torch.zeros(len(modes), nx, ny, device='cuda')
    st = s.init(z, z)
    assert float(st.what.abs().max()) == 0.0
    for b, (m, j) in enumerate(modes):
        st.what[b, j, m % nx, 0], st.what[b, j, m % nx, 1] = 0.75, -1.25
        if j == 0:
            st.what[b, 0, (-m) % nx, 0], st.what[b, 0, (-m) % nx, 1] = 0.75, 1.25
    sp = s.spectrum(st)
    E, Z = npy(sp.energy), npy(sp.enstrophy)
    S = len(sp.k)
    pos = PO.shell_position(T)
    for b, (m, j) in enumerate(modes):
        want = int(np.floor(pos[m % nx, j]))
        assert E[b, want] >= (1 - 1e-10) * E[b].sum() > 0 and Z[b, want] >= (1 - 1e-10) * Z[b].sum() > 0, (m, j, want)
        assert np.count_nonzero(E[b]) == 1
        if j == my1 - 1:
            assert want == S - 1
    n2 = float(nx * ny) ** 2
    assert abs(Z[0].sum() / (2 * 0.5 * (0.75 ** 2 + 1.25 ** 2) / n2) - 1) <= 1e-6          # weight 2 off the j = 0 line, float32 inputs


# ---------------------------------------------------------------------------------------------------- 3. transfer
@pytest.mark.parametrize('case', PC.CASES, ids=IDS)
def test_transfer_against_the_oracle_of_the_same_state(gpu_device, case):
    # one float32 evaluation of the nonlinear term against the float64 one of the same state; PC.BOUND_TRANSFER and the figures
    # measured on the MI355X are in tests/pspec_spectrum_cases.py, the wrong definitions the bound catches in tests/test_oracle_pspec_spectrum.py
    nx, ny, B, Lx, Ly, _ = case
    s, st, T, w, t = case_run(case)
    ref = PO.transfer(T, w, t)
    tr = s.transfer(st)
    S = len(tr.k)
    assert tr._fields == ('k', 'energy', 'enstrophy', 'variance') and np.array_equal(tr.k, s.shells()[0])
    assert all(x.dtype == torch.float64 and tuple(x.shape) == (B, S) for x in tr[1:])
    errs, sums = {}, {}
    for name, got, a in (('T_E', tr.energy, 'A_E'), ('T_Z', tr.enstrophy, 'A_Z'), ('T_theta', tr.variance, 'A_theta')):
        got = npy(got)
        errs[name] = (np.abs(got - ref[name]).sum(-1) / ref[a].sum(-1)).max()
        sums[name] = (np.abs(got.sum(-1)) / ref[a].sum(-1)).max()
        assert (got[:, 0] == 0).all()
    rhs, scale = PO.energy_budget(T, w)
    eb = (np.abs(npy(s.energy_budget(st)) - rhs).sum(-1) / scale.sum(-1)).max()
    print('transfer %dx%d B=%d S=%d: sum_s |T - oracle| / sum_s A: T_E %.2e T_Z %.2e T_theta %.2e; |sum_s T| / sum_s A: %.2e %.2e %.2e; budget %.2e'
          % (nx, ny, B, S, errs['T_E'], errs['T_Z'], errs['T_theta'], sums['T_E'], sums['T_Z'], sums['T_theta'], eb))
    assert max(errs.values()) <= PC.BOUND_TRANSFER, errs
    assert max(sums.values()) <= PC.BOUND_TRANSFER, sums
    assert eb <= PC.BOUND_TRANSFER, eb
    # the flux closes: Pi(S - 1) = -sum_s T
    from nns.periodic import flux
    pi = flux(tr.energy)
    assert tuple(pi.shape) == (B, S) and torch.equal(pi[:, 0], -tr.energy[:, 0])
    assert (np.abs(npy(pi[:, -1])) / ref['A_E'].sum(-1)).max() <= PC.BOUND_TRANSFER


# ---------------------------------------------------------------------------------------------------- 4. contracts
def test_spectrum_and_transfer_only_read_the_state(gpu_device):
    case = PC.CASES[0]
    s, st0, T, w, t = case_run(case)
    st = st0.clone()
    keep = [x.clone() for x in (st.what, st.that, st.mean)]
    steps = st.steps
    sp, tr, bu = s.spectrum(st), s.transfer(st), s.energy_budget(st)
    assert all(torch.equal(a, b) for a, b in zip(keep, (st.what, st.that, st.mean))) and st.steps == steps
    # repeated calls are bitwise equal
    for a, b in zip(sp[1:] + tr[1:], s.spectrum(st)[1:] + s.transfer(st)[1:]):
        assert torch.equal(a, b)
    assert torch.equal(bu, s.energy_budget(st))
    # a state stepped after a transfer call is the state stepped without one
    other = st0.clone()
    s.step(st, 1), s.step(other, 1)
    assert torch.equal(st.what, other.what) and torch.equal(st.that, other.that) and not torch.equal(st.what, keep[0])


@pytest.mark.parametrize('case', [PC.CASES[0], PC.CASES[3]], ids=[IDS[0], IDS[3]])
def test_a_grid_of_a_batch_gives_the_numbers_of_the_grid_alone(gpu_device, case):
    nx, ny, B, Lx, Ly, _ = case
    s, st, T, w, t = case_run(case)
    sp, tr = s.spectrum(st), s.transfer(st)
    z = torch.zeros(1, nx, ny, device='cuda')
    for b in range(B):
        one = s.init(z, z, z)
        one.what.copy_(st.what[b:b + 1]), one.that.copy_(st.that[b:b + 1]), one.mean.copy_(st.mean[b:b + 1])
        for a, c in zip(sp[1:] + tr[1:], s.spectrum(one)[1:] + s.transfer(one)[1:]):
            assert torch.equal(a[b], c[0])
    assert not torch.equal(sp.energy[0], sp.energy[1])


def test_the_mean_flow_transfers_nothing(gpu_device):
    s, st0, T, w, t = case_run(PC.CASES[0])
    assert float(st0.mean.abs().min()) > 0.1
    still = st0.clone()
    still.mean.zero_()
    for a, b in zip(s.transfer(st0)[1:], s.transfer(still)[1:]):
        assert torch.equal(a, b)


def test_a_state_without_a_scalar_and_a_force_of_another_batch(gpu_device):
    from nns import ops
    from nns.periodic import PeriodicSolver
    case = PC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    s, st, T, w, t = case_run(case)
    u0, v0 = PC.reference(case)[1:3]
    flow = s.init(dev(u0), dev(v0))
    flow.what.copy_(st.what)
    sp, tr = s.spectrum(flow), s.transfer(flow)
    assert sp.variance is None and tr.variance is None
    full, ftr = s.spectrum(st), s.transfer(st)
    assert torch.equal(sp.energy, full.energy) and torch.equal(sp.injection, full.injection)
    assert torch.equal(tr.energy, ftr.energy) and torch.equal(tr.enstrophy, ftr.enstrophy)          # the flow's transfer does not see the scalar
    raw = ops.spec_ns_spectrum(flow.what, None, s.ghat, ny, Lx, Ly, out=torch.full((B, 4, len(sp.k)), 7.0, dtype=torch.float64, device='cuda'))
    assert float(raw[:, 3].abs().max()) == 0.0 and torch.equal(raw[:, 0], sp.energy)
    rawt = ops.spec_ns_transfer(flow.what, None, flow.work, ny, Lx, Ly, out=torch.full((B, 3, len(sp.k)), 7.0, dtype=torch.float64, device='cuda'))
    assert float(rawt[:, 2].abs().max()) == 0.0 and torch.equal(rawt[:, 1], tr.enstrophy)
    # without a force the injection is zeros
    plain = PeriodicSolver(nx, ny, s.dt, C.RHO, C.NU, Lx=Lx, Ly=Ly)
    assert float(plain.spectrum(flow).injection.abs().max()) == 0.0
    # a per-grid force of another batch is refused before any launch
    fx, fy = FC.random_forces(2, nx, ny, 5, Lx, Ly)
    per_grid = PeriodicSolver(nx, ny, s.dt, C.RHO, C.NU, Lx=Lx, Ly=Ly).set_forcing(dev(fx), dev(fy))
    with pytest.raises(ValueError, match='per grid'):
        per_grid.spectrum(flow)
    with pytest.raises(ValueError, match='per grid'):
        per_grid.energy_budget(flow)
    # a per-grid force of the state's batch is taken grid by grid
    fx, fy = FC.random_forces(B, nx, ny, 6, Lx, Ly)
    per_grid.set_forcing(dev(fx), dev(fy))
    F = npy(per_grid.spectrum(flow).injection)
    T2 = SC.scheme(nx, ny, s.dt, Lx, Ly)
    T2.g = T2.expand(state_c(per_grid.ghat))
    ref = PO.spectrum(T2, w)
    assert (np.abs(F - ref['F']).sum(-1) / ref['A_F'].sum(-1)).max() <= PC.BOUND_SPECTRUM
    assert np.abs(npy(per_grid.diagnostics(flow).power_in) / F.sum(-1) - 1).max() <= PC.BOUND_SPECTRUM


def test_transfer_is_capturable(gpu_device):
    from nns import ops
    case = PC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    s, st0, T, w, t = case_run(case)
    st = st0.clone()
    eager = ops.spec_ns_transfer(st.what, st.that, st.work, ny, Lx, Ly)          # first launches outside the capture
    sp = ops.spec_ns_spectrum(st.what, st.that, s.ghat, ny, Lx, Ly)
    out, out2 = torch.zeros_like(eager), torch.zeros_like(sp)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.spec_ns_transfer(st.what, st.that, st.work, ny, Lx, Ly, out=out)
        ops.spec_ns_spectrum(st.what, st.that, s.ghat, ny, Lx, Ly, out=out2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out2, sp)


# ---------------------------------------------------------------------------------------------------- 5. error codes
def test_error_codes(gpu_device):
    from nns import ops, _lib
    L = _lib.lib()
    B, nx, ny, my1, S = 3, 64, 64, 22, 31
    what = torch.zeros(B, my1, nx, 2, device='cuda')
    that = torch.zeros(B, my1, nx, 2, device='cuda')
    g = torch.zeros(B, my1, nx, 2, device='cuda')
    ns = ops.spec_ns_scalar_workspace(B, nx, ny)
    work = torch.empty(ns, dtype=torch.uint8, device='cuda')
    out = torch.empty(B, 4, S, dtype=torch.float64, device='cuda')
    p = lambda x: x.data_ptr()
    assert ops.spec_ns_shells(nx, ny, TWO_PI, TWO_PI) == (S, 1.0)

    def spectrum(w=p(what), t=p(that), gh=None, gb=0, o=p(out), nshell=S, batch=B, nx=nx):
        return L.nns_spec_ns_spectrum_f32(w, t, gh, gb, o, nshell, batch, nx, ny, TWO_PI, TWO_PI, None)
    assert spectrum(w=None) == INVALID and spectrum(o=None) == INVALID and spectrum(batch=0) == INVALID
    assert spectrum(nshell=S - 1) == INVALID and b'nshell' in L.nns_last_error() and spectrum(nshell=S + 1) == INVALID
    assert spectrum(gh=p(g), gb=2) == INVALID and spectrum(gh=None, gb=1) == INVALID
    assert spectrum(nx=96) == UNSUPPORTED
    assert spectrum() == 0 and spectrum(t=None) == 0 and spectrum(gh=p(g), gb=B) == 0 and spectrum(gh=p(g), gb=1) == 0

    def transfer(w=p(what), t=p(that), o=p(out), nshell=S, wk=p(work), wb=ns, batch=B, nx=nx):
        return L.nns_spec_ns_transfer_f32(w, t, o, nshell, wk, wb, batch, nx, ny, TWO_PI, TWO_PI, None)
    assert transfer(w=None) == INVALID and transfer(o=None) == INVALID and transfer(wk=None) == INVALID and transfer(batch=0) == INVALID
    assert transfer(nshell=S - 1) == INVALID and b'nshell' in L.nns_last_error()
    assert transfer(nx=96) == UNSUPPORTED
    assert transfer(wb=ns - 1) == WORKSPACE and b'nns_spec_ns_scalar_workspace' in L.nns_last_error()
    assert transfer(t=None, wb=ops.spec_ns_workspace(B, nx, ny) - 1) == WORKSPACE
    assert transfer() == 0 and transfer(t=None) == 0 and transfer(t=None, wb=ops.spec_ns_workspace(B, nx, ny)) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0          # a zero state has no spectrum and transfers nothing
    n, dk = ctypes.c_int(0), ctypes.c_double(0.0)
    assert L.nns_spec_ns_shells(nx, ny, TWO_PI, TWO_PI, None, ctypes.byref(dk)) == INVALID
    assert L.nns_spec_ns_shells(96, ny, TWO_PI, TWO_PI, ctypes.byref(n), ctypes.byref(dk)) == UNSUPPORTED
    # host: refused before any launch
    with pytest.raises(ValueError):
        ops.spec_ns_spectrum(what, that[:2], None, ny, TWO_PI, TWO_PI)
    with pytest.raises(ValueError):
        ops.spec_ns_spectrum(what, None, None, ny, TWO_PI, TWO_PI, out=torch.empty(B, 3, S, dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError):
        ops.spec_ns_transfer(what, None, work, 128, TWO_PI, TWO_PI)
    with pytest.raises(TypeError):
        ops.spec_ns_transfer(what, None, work.float(), ny, TWO_PI, TWO_PI)
    with pytest.raises(_lib.NnsError, match='workspace'):
        ops.spec_ns_transfer(what, that, work[:-1], ny, TWO_PI, TWO_PI)
    from nns.periodic import PeriodicSolver
    with pytest.raises(TypeError):
        PeriodicSolver(64, 64, 0.01, 1.0, 0.0).spectrum(what)
