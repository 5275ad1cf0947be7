"""CPU checks of tests/pspec_spectrum_oracle.py, the float64 restatement of the shell spectra and spectral transfers of the periodic spectral
solver: its shell sums are the totals of the restatements it is built on, its transfers conserve, its budget is the time derivative of E(s), the
bounds of tests/pspec_spectrum_cases.py would catch every wrong definition listed there, and the three C entry points refuse bad arguments before
any HIP call."""
import ctypes
import os

import numpy as np
import pytest

import pspec_cases as C
import pspec_forced_cases as FC
import pspec_oracle as O
import pspec_scalar_cases as SC
import pspec_spectrum_cases as PC
import pspec_spectrum_oracle as PO

IDS = [C.case_id(c) for c in PC.CASES]
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
SHELLS = dict(zip(IDS, (31, 240, 346, 343, 343)))


@pytest.mark.parametrize('case', PC.CASES, ids=IDS)
def test_shell_sums_are_the_totals(case):
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0, w, t, mean = PC.reference(case)
    k, dk, n = PO.shells(nx, ny, Lx, Ly)
    assert n == SHELLS[C.case_id(case)] and len(k) == n and dk == min(2 * np.pi / Lx, 2 * np.pi / Ly) and np.allclose(k, dk * np.arange(n))
    sp = PO.spectrum(S, w, t)
    E, Z, P = S.diag(w)
    # Scheme.energy is the physical-space mean of (u^2 + v^2) / 2, the mean flow included; Scheme.enstrophy that of w^2 / 2
    e_phys = S.energy(w, mean) - 0.5 * (mean ** 2).sum(axis=-1)
    errs = [np.abs(sp['E'].sum(-1) / e_phys - 1).max(), np.abs(sp['Z'].sum(-1) / S.enstrophy(w) - 1).max(), np.abs(sp['F'].sum(-1) / P - 1).max(),
            np.abs(sp['V'].sum(-1) / S.scalar_diag(w, t)[0] - 1).max(), np.abs(sp['E'].sum(-1) / E - 1).max()]
    print('shell sums %s: E (physical), Z (physical), F, V, E (Parseval) relative to the totals %s' % (IDS[PC.CASES.index(case)], ['%.1e' % e for e in errs]))
    assert max(errs) <= 1e-13, errs
    assert (sp['E'] >= 0).all() and (sp['Z'] >= 0).all() and (sp['V'] >= 0).all()
    assert (sp['E'][..., 0] == 0).all() and (sp['E'][..., -1] > 0).all()          # shell 0 is empty, the corner's shell is the last
    assert PO.spectrum(S, w)['V'] is None


@pytest.mark.parametrize('case', PC.CASES, ids=IDS)
def test_transfers_sum_to_zero(case):
    S, u0, v0, th0, w, t, mean = PC.reference(case)
    tr = PO.transfer(S, w, t)
    r = [np.abs(tr[a].sum(-1)).max() / tr[b].sum(-1).min() for a, b in (('T_E', 'A_E'), ('T_Z', 'A_Z'), ('T_theta', 'A_theta'))]
    print('sum_s T / sum_s A %s: %s' % (C.case_id(case), ['%.1e' % x for x in r]))
    assert max(r) <= 1e-13, r
    # and the transfers are there to be compared: a tenth of their scale
    assert min(np.abs(tr[a]).sum() / tr[b].sum() for a, b in (('T_E', 'A_E'), ('T_Z', 'A_Z'), ('T_theta', 'A_theta'))) >= 0.05


@pytest.mark.parametrize('case', PC.CASES, ids=IDS)
def test_forced_damped_budget_is_the_time_derivative(case):
    # E(s) a step h before and after the state, by the scheme itself (RK4: its own error h^4 is far below); the central difference is
    # second order, so halving h divides its distance from the budget by 4
    nx, ny, B, Lx, Ly, _ = case
    S, u0, v0, th0, w, t, mean = PC.reference(case)
    rhs, scale = PO.energy_budget(S, w)
    errs = []
    for div in (4, 8):
        h = S.dt / div
        E = []
        for sgn in (-1.0, 1.0):
            T = FC.scheme(nx, ny, sgn * h, Lx, Ly).kolmogorov_forcing(FC.KF, FC.AMP)
            E.append(PO.spectrum(T, T.step(w, mean, 1))['E'])
        errs.append(np.abs((E[1] - E[0]) / (2 * h) - rhs).sum(-1).max() / scale.sum(-1).min())
    print('budget against the central difference %s: h = dt/4 %.2e, dt/8 %.2e, ratio %.2f' % (C.case_id(case), errs[0], errs[1], errs[0] / errs[1]))
    assert errs[0] <= 2e-3 and 3.0 <= errs[0] / errs[1] <= 5.0, errs
    # every term of the budget takes part
    sp = PO.spectrum(S, w)
    assert min(np.abs(x).sum() for x in (sp['F'], 2 * S.nu * sp['Z'], 2 * S.drag * sp['E'])) >= 1e-4 * scale.sum()


def _affected(mutation, case):
    """The quantities a mutation must move, or None where it is the identity: dk = max on a box with Lx = Ly, which is three of the five
    cases (the two widths differ on 128x512 and 512x128 only)."""
    if mutation == 'dkmax' and case[3] == case[4]:
        return None
    return {'floor': ('T_E', 'T_Z', 'T_theta', 'E', 'Z', 'V'), 'weight1': ('T_E', 'T_Z', 'T_theta', 'E', 'Z', 'F', 'V'),
            'dkmax': ('T_E', 'T_Z', 'T_theta', 'E', 'Z', 'V'), 'noik2': ('T_E', 'E', 'F'), 'sign': ('T_E', 'T_Z', 'T_theta'),
            'grad': ('T_theta',)}[mutation]


@pytest.mark.parametrize('mutation', PO.MUTATIONS)
@pytest.mark.parametrize('case', PC.CASES, ids=IDS)
def test_the_bounds_catch_wrong_definitions(case, mutation):
    # the measures of tests/test_gpu_pspec_spectrum.py, taken between the restatement and a wrong one: each must be >= 100x the bound there
    S, u0, v0, th0, w, t, mean = PC.reference(case)
    sp, tr = PO.spectrum(S, w, t), PO.transfer(S, w, t)
    msp, mtr = PO.spectrum(S, w, t, mutation), PO.transfer(S, w, t, mutation)
    scale = dict(T_E='A_E', T_Z='A_Z', T_theta='A_theta')
    moved = {}
    for q in ('T_E', 'T_Z', 'T_theta'):
        moved[q] = (np.abs(mtr[q] - tr[q]).sum(-1) / tr[scale[q]].sum(-1)).min() / PC.BOUND_TRANSFER
    for q in ('E', 'Z', 'V'):
        live = sp[q] > 0
        moved[q] = np.abs(msp[q][live] / sp[q][live] - 1).max() / PC.BOUND_SPECTRUM
    moved['F'] = (np.abs(msp['F'] - sp['F']) / sp['A_F'].sum(-1, keepdims=True)).max() / PC.BOUND_SPECTRUM
    affected = _affected(mutation, case)
    print('%s %s: moved by (in units of the bound) %s' % (mutation, C.case_id(case), {q: '%.1e' % v for q, v in moved.items()}))
    if affected is None:
        assert max(moved.values()) == 0.0
        return
    for q in affected:
        assert moved[q] >= 100.0, (q, moved[q])
    for q in moved:
        if q not in affected and not (q == 'F' and mutation in ('floor', 'dkmax')):          # the force's one mode may or may not change shell
            assert moved[q] == 0.0, (q, moved[q])


def _lib():
    from nns import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_shell_count_of_the_library_is_the_restatements():
    L = _lib()
    for nx, ny, B, Lx, Ly, _ in PC.CASES + [(512, 512, 1, C.TWO_PI, C.TWO_PI, None), (1024, 1024, 1, 3.0, 0.5, None)]:
        n, dk = ctypes.c_int(0), ctypes.c_double(0.0)
        assert L.nns_spec_ns_shells(nx, ny, Lx, Ly, ctypes.byref(n), ctypes.byref(dk)) == 0
        k, odk, S = PO.shells(nx, ny, Lx, Ly)
        assert n.value == S and dk.value == odk, (nx, ny, n.value, S)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """No GPU here: every call below must return from its argument checks (a launch or a device query would fail or fault on the host
    pointers).  Fails where the symbols are missing."""
    L = _lib()
    n, dk = ctypes.c_int(0), ctypes.c_double(0.0)
    assert L.nns_spec_ns_shells(64, 64, C.TWO_PI, C.TWO_PI, None, ctypes.byref(dk)) == INVALID
    assert L.nns_spec_ns_shells(64, 64, C.TWO_PI, C.TWO_PI, ctypes.byref(n), None) == INVALID
    assert L.nns_spec_ns_shells(64, 64, 0.0, C.TWO_PI, ctypes.byref(n), ctypes.byref(dk)) == INVALID
    assert L.nns_spec_ns_shells(96, 64, C.TWO_PI, C.TWO_PI, ctypes.byref(n), ctypes.byref(dk)) == UNSUPPORTED
    assert L.nns_spec_ns_shells(64, 2048, C.TWO_PI, C.TWO_PI, ctypes.byref(n), ctypes.byref(dk)) == UNSUPPORTED
    assert L.nns_spec_ns_shells(64, 64, C.TWO_PI, C.TWO_PI, ctypes.byref(n), ctypes.byref(dk)) == 0 and n.value == 31 and dk.value == 1.0
    host = (ctypes.c_double * 64)()                       # stands for every device pointer: never dereferenced
    p = ctypes.addressof(host)
    big = 1 << 40

    def spectrum(what=p, that=p, ghat=None, gbatch=0, out=p, nshell=31, batch=3, nx=64, Lx=C.TWO_PI):
        return L.nns_spec_ns_spectrum_f32(what, that, ghat, gbatch, out, nshell, batch, nx, 64, Lx, C.TWO_PI, None)
    assert spectrum(what=None) == INVALID and spectrum(out=None) == INVALID and spectrum(batch=0) == INVALID
    assert spectrum(nshell=30) == INVALID and b'nshell' in L.nns_last_error()
    assert spectrum(nshell=32) == INVALID and spectrum(nshell=0) == INVALID
    assert spectrum(ghat=p, gbatch=2) == INVALID and b'gbatch' in L.nns_last_error()
    assert spectrum(ghat=None, gbatch=1) == INVALID and spectrum(ghat=p, gbatch=0) == INVALID
    assert spectrum(Lx=-1.0) == INVALID and spectrum(nx=96) == UNSUPPORTED

    def transfer(what=p, that=p, out=p, nshell=31, work=p, wb=big, batch=3, nx=64, Lx=C.TWO_PI):
        return L.nns_spec_ns_transfer_f32(what, that, out, nshell, work, wb, batch, nx, 64, Lx, C.TWO_PI, None)
    assert transfer(what=None) == INVALID and transfer(out=None) == INVALID and transfer(work=None) == INVALID and transfer(batch=0) == INVALID
    assert transfer(nshell=30) == INVALID and b'nshell' in L.nns_last_error()
    assert transfer(nshell=32, that=None) == INVALID
    assert transfer(Lx=float('nan')) == INVALID and transfer(nx=96) == UNSUPPORTED
    need = ctypes.c_size_t(0)
    assert L.nns_spec_ns_scalar_workspace(3, 64, 64, ctypes.byref(need)) == 0
    assert transfer(wb=need.value - 1) == WORKSPACE and b'nns_spec_ns_scalar_workspace' in L.nns_last_error()
    assert L.nns_spec_ns_workspace(3, 64, 64, ctypes.byref(need)) == 0
    assert transfer(that=None, wb=need.value - 1) == WORKSPACE and b'nns_spec_ns_workspace' in L.nns_last_error()
