"""The cases of the spectral residual backward (tests/specbwd_cases.py; tests/test_gpu_specbwd.py holds the HIP kernels to them), on the reference
alone: the formula the wrong oracles are cut from is the oracle, every wrong oracle misses every bound by >= 100 x, the float32 evaluation of
the reference stays under 2e-6, and each case reaches the part of the dispatch it is there for."""
import math

import numpy as np
import pytest
import torch

import specbwd_cases as SC
from specbwd_cases import rel_l2

SHAPES = sorted({(c.B, c.nx, c.ny, c.A, c.swap) for c in SC.CASES})


def test_the_case_list_is_the_one_agreed():
    assert len(SC.CASES) == 75 and len(set(SC.CASES)) == 75
    for N in SC.FFT_LENGTHS:
        for p in (0, 2):
            assert any(c[:4] == (2, N, 100, p) for c in SC.CASES) and any(c[:4] == (3, 7, N, p) for c in SC.CASES)
    for s in ((2, 64, 1024), (1, 1024, 64), (1, 128, 512), (1, 512, 128), (1, 256, 256)):
        assert {c.precise for c in SC.CASES if c[:3] == s} == {0, 2}
    assert {(c.precise, c.A) for c in SC.CASES} == {(0, 0.1), (0, 4.0), (2, 0.1), (2, 4.0), (2, 20.0)}
    assert [m[0][:4] for m in SC.MULTI] == [(1100, 64, 64, 0), (140, 1024, 64, 0), (280, 256, 100, 0), (600, 7, 1024, 2), (601, 7, 1024, 2),
                                            (140, 1024, 64, 2)]
    assert len(SC.GUARD_CASES) == 8 and len(SC.MUTATIONS) == 8
    assert max(c.B * c.nx * c.ny for c, _, _ in SC.MULTI) == 140 * 1024 * 64            # the largest anything allocates: 9.2 M points per field
    for c in SC.CASES:
        dt, Lx, Ly, rho, nu = SC.params(c)
        assert (dt, rho) == (1.0, 1.3) and {Lx, Ly} == {1.5, 4.0} and (Lx == 4.0) == c.swap
        n, L = max(((c.nx, Lx), (c.ny, Ly)), key=lambda t: t[0] / t[1])
        assert abs(SC.amplification(nu, n, L) - c.A) < 1e-12 and SC.is_fft(n)             # the axis that sets nu is an FFT axis in every case


def test_inputs_follow_the_recipe():
    """max-abs 1 per field and grid, float32, energy on both Nyquist lines, the same grid whatever batch it is asked for in, and a (1 + |m|)^-1
    spectrum: the mean |F|^2 (1 + |m|)^2 over the wavenumber shells is flat to a factor of 2 from |m| = 4 to the Nyquist line."""
    c = SC.Case(2, 128, 100, 0, 4.0, False)
    f = SC.fields(c)
    assert len(f) == 5 and all(t.dtype == torch.float32 and t.shape == (2, 128, 100) for t in f)
    for t in f:
        assert torch.equal(t.abs().amax(dim=(1, 2)), torch.ones(2))
    assert all(torch.equal(a[1:], b) for a, b in zip(f, SC.fields(c, grids=(1,))))
    assert not torch.equal(f[0][0], f[0][1]) and not torch.equal(f[0], f[1])
    F = np.fft.fft2(f[0][0].double().numpy())
    assert np.abs(F[64, :]).mean() > 0.02 * np.abs(F[1:, 1:]).mean() and np.abs(F[:, 50]).mean() > 0.02 * np.abs(F[1:, 1:]).mean()
    big = SC.make_fields(256, 256, (0,))[0][0].double().numpy()
    P = np.abs(np.fft.fft2(big)) ** 2
    m = np.hypot(np.fft.fftfreq(256, 1 / 256)[:, None], np.fft.fftfreq(256, 1 / 256)[None, :])
    shell = [float((P * (1 + m) ** 2)[(m >= lo) & (m < 2 * lo)].mean()) for lo in (4, 8, 16, 32, 64)]
    assert max(shell) < 2 * min(shell), shell


@pytest.mark.parametrize('B,nx,ny,A,swap', SHAPES, ids=['B%d-%dx%d-A%g%s' % (s[:4] + ('-swap' if s[4] else '',)) for s in SHAPES])
def test_bounds_reject_the_wrong_oracles(B, nx, ny, A, swap):
    """Per shape and amplification (the inputs do not depend on `precise`; the bound does): `vjp` in float64 is the oracle, its float32
    evaluation is within 2e-6 of it, and every wrong oracle that applies misses the bound of both arithmetics by >= 100 x in some output."""
    cases = [c for c in SC.CASES if (c.B, c.nx, c.ny, c.A, c.swap) == (B, nx, ny, A, swap)]
    assert {c.precise for c in cases} == ({0, 2} if A <= SC.AMP_MAX else {2})
    ref = SC.oracle(cases[0])
    same = SC.vjp(SC.fields(cases[0]), SC.params(cases[0]))
    assert all(rel_l2(same[q], ref[q]) < 1e-13 for q in SC.OUTPUTS)
    assert all(ref[q].shape == (B, nx, ny) and np.abs(ref[q]).max() > 0 for q in SC.ALL_OUTPUTS)
    e = SC.e32(cases[0])
    bounds = {c.precise: SC.bound(c) for c in cases}
    print('specbwd case B%d-%dx%d-A%g: e32 %.2e, bounds %s' % (B, nx, ny, A, e, bounds))
    assert 0 < e <= SC.E32_LIMIT, e
    for p, bd in bounds.items():
        assert bd == (1e-5 if p == 0 else min(1e-5, max(10 * e, 1e-6)))
    dt, Lx, Ly, rho, nu = SC.params(cases[0])
    applied = 0
    for mutation in SC.MUTATIONS:
        if not SC.mutation_applies(mutation, nx, Lx, ny, Ly):
            continue
        applied += 1
        bad = SC.mutant(mutation, cases[0])
        moved = {q: rel_l2(bad[q], ref[q]) for q in SC.OUTPUTS}
        print('  %-15s %s' % (mutation, '  '.join('%s %.2e' % kv for kv in moved.items())))
        assert max(moved.values()) >= 100 * max(bounds.values()), (mutation, moved, bounds)
    assert applied == 8                                           # Lx != Ly and an FFT axis in every case


def test_cases_reach_the_dispatch_they_are_there_for():
    """The kernel constants restated (LINES = 8192 / N, at most 512 workgroups, float32 up to amplification 8): which kernels a case launches,
    that the x-pass cases end on a ragged column tile and the y-pass cases on a partial row group, in both arithmetics and at every N."""
    assert [SC.lines(n) for n in SC.FFT_LENGTHS] == [128, 64, 32, 16, 8]
    seen = set()
    for c in SC.CASES:
        d = SC.dispatch(c)
        amp = {'x': d['amp_x'], 'y': d['amp_y']}
        fft_axes = [ax for ax, n in (('x', c.nx), ('y', c.ny)) if SC.is_fft(n)]
        assert abs(max(amp[ax] for ax in fft_axes) - c.A) < 1e-12
        assert d['f32'] == (c.precise == 0)
        if c.precise == 0:
            assert all(amp[ax] <= SC.AMP_MAX for ax in fft_axes)                  # the float32 mode is tested only where it is legitimate
        if c.A == 20.0:
            assert c.precise == 2 and any(amp[ax] > SC.AMP_MAX for ax in fft_axes)
        for ax in ('x', 'y'):
            k = d[ax]['kernel']
            assert (k == 'dense') == (ax not in fft_axes)
            if k != 'dense':
                assert k.endswith('f32' if c.precise == 0 else 'f64') and d[ax]['max_per_workgroup'] == 1
                seen.add((k, d[ax]['lines']))
        if (c.B, c.ny) == (2, 100):
            assert d['x']['ragged'] and d['x']['tiles_per_grid'] == -(-100 // (8192 // c.nx)) and d['y']['kernel'] == 'dense'
        if (c.B, c.nx) == (3, 7):
            assert d['y']['partial_tail'] and d['y']['rows'] == 21 and d['x']['kernel'] == 'dense'
    assert seen == {(k, w) for k in ('xsplit_f32', 'xpass_f64', 'ypass_f32', 'ypass_f64') for w in (128, 64, 32, 16, 8)}
    for c in SC.GUARD_CASES:
        d = SC.dispatch(c)
        assert d['x'].get('ragged') or d['y'].get('partial_tail')
    assert {(c.nx if c.ny == 100 else c.ny, c.precise) for c in SC.GUARD_CASES} == {(64, 0), (64, 2), (1024, 0), (1024, 2)}


def test_the_precise_policy_restated():
    """precise = 1 at A = 4 resolves to float32 and at A = 20 to float64; the anisotropic case exceeds 8 along y only and resolves to float64."""
    for shape in SC.POLICY_SHAPES:
        for A, f32 in ((4.0, True), (20.0, False)):
            c = SC.Case(*shape, 1, A, False)
            assert SC.dispatch(c)['f32'] == f32
    B, nx, ny = SC.ANISO_SHAPE
    L = SC.ANISO_L
    nu = SC.ANISO_AMP_Y * math.sqrt(3.0) * L / (math.pi * ny)
    assert SC.amplification(nu, ny, L) > SC.AMP_MAX > 1.0 > SC.amplification(nu, nx, L)
    assert not SC.resolved_f32(1, nu, nx, L, ny, L) and SC.resolved_f32(1, nu, nx, L, 100, L) and SC.resolved_f32(0, nu, nx, L, ny, L)


def test_multi_tile_cases_give_a_workgroup_a_third_tile():
    for c, which, what in SC.MULTI:
        d = SC.dispatch(c)
        p = d[which]
        assert p['kernel'] == {('x', 0): 'xsplit_f32', ('x', 2): 'xpass_f64', ('y', 2): 'ypass_f64'}[(which, c.precise)], what
        assert p['workgroups'] == SC.GRID_CAP and p['tiles'] % SC.GRID_CAP != 0
        if (c.nx, c.ny) == (7, 1024):
            # rows in groups of 8: a second iteration for 13 / 14 workgroups; 4200 rows end on a full group, 4207 on one of 7 rows (the three-deep
            # float64 row loop: below)
            assert p['tiles'] == {600: 525, 601: 526}[c.B] and p['max_per_workgroup'] == 2 and d['x']['kernel'] == 'dense'
            assert p['partial_tail'] == (c.B == 601) and p['rows'] % 8 == {600: 0, 601: 7}[c.B]
        else:
            assert p['tiles'] > 2 * SC.GRID_CAP and p['max_per_workgroup'] >= 3, what
        # the chunks of the bitwise comparison: consecutive, covering, no second tile for any workgroup in either pass, first boundary odd
        ch = SC.chunks(c)
        assert ch[0][0] == 0 and ch[-1][1] == c.B and all(a[1] == b[0] for a, b in zip(ch, ch[1:])) and ch[0][1] % 2 == 1 and len(ch) >= 2
        for b0, b1 in ch:
            dd = SC.dispatch(c._replace(B=b1 - b0))
            assert all(dd[ax].get('max_per_workgroup', 1) == 1 for ax in ('x', 'y')), (c, b0, b1)
        g = SC.compared_grids(c)
        assert len(g) == 3 and g[0] == 0 and g[-1] == c.B - 1
    by = {SC.case_id(c): SC.dispatch(c) for c, _, _ in SC.MULTI}
    a = by['B1100-64x64-p0-A4']
    assert (a['x']['tiles'], a['x']['lines'], a['x']['ragged'], a['y']['tiles']) == (1100, 128, True, 550)
    b = by['B140-1024x64-p0-A4']
    assert (b['x']['tiles'], b['x']['lines'], b['y']['tiles'], b['y']['kernel']) == (1120, 8, 1120, 'ypass_f32')
    m = by['B280-256x100-p0-A4']
    assert (m['x']['tiles'], m['x']['tiles_per_grid'], m['x']['ragged'], m['y']['kernel']) == (1120, 4, True, 'dense')
    f = by['B140-1024x64-p2-A20']
    assert (f['x']['tiles'], f['y']['tiles'], f['y']['kernel'], f['y']['max_per_workgroup']) == (1120, 1120, 'ypass_f64', 3)


@pytest.mark.parametrize('k', range(len(SC.MULTI)), ids=[SC.case_id(m[0]) for m in SC.MULTI])
def test_multi_tile_bounds_reject_the_wrong_oracles(k):
    """The three grids of a multi-tile call that are compared with the oracle: the same conditions as for the small cases."""
    c = SC.MULTI[k][0]
    g = tuple(SC.compared_grids(c))
    ref, e, bd = SC.oracle(c, g), SC.e32(c, g), SC.bound(c, g)
    print('specbwd multi %s: e32 %.2e, bound %.2e' % (SC.case_id(c), e, bd))
    assert 0 < e <= SC.E32_LIMIT
    assert bd == (1e-5 if c.precise == 0 else min(1e-5, max(10 * e, 1e-6)))
    dt, Lx, Ly, rho, nu = SC.params(c)
    for mutation in SC.MUTATIONS:
        assert SC.mutation_applies(mutation, c.nx, Lx, c.ny, Ly)
        bad = SC.mutant(mutation, c, g)
        assert max(rel_l2(bad[q], ref[q]) for q in SC.OUTPUTS) >= 100 * bd, mutation


def test_single_mode_setups():
    """The analytic cases: the Nyquist mode is (-1)^j along its axis, the oracle gives grad_p = 0 and grad_u = (1 / dt + nu k_N^2) g_u for it,
    and on the leak probe the packed-Nyquist mutant -- what the probe is for -- moves grad_u and grad_v by more than the outputs' own size."""
    for N, axis, _ in SC.NYQUIST_CASES[::2]:
        shape, prm, mode, k_n = SC.nyquist_setup(N, axis)
        assert mode.shape == shape and torch.equal(mode.abs(), torch.ones(shape))
        z = torch.zeros(shape)
        ref = SC.oracle_of((z, z, mode, z, z), prm)
        assert np.abs(ref['grad_p']).max() < 1e-9 * k_n
        assert rel_l2(ref['grad_u'], (1.0 / prm[0] + prm[4] * k_n ** 2) * mode.double().numpy()) < 1e-12
        assert np.abs(ref['grad_v']).max() == 0
        prm, f = SC.leak_probe(N, axis)
        ref = SC.oracle_of(f, prm)
        bad = SC.vjp(f, prm, torch.float64, 'nyquist_packed')
        assert rel_l2(bad['grad_v'], ref['grad_v']) > 1 and (axis == 'y' or rel_l2(bad['grad_u'], ref['grad_u']) > 1)     # along y only g_v v_y sees u
        same = SC.vjp(f, prm)
        assert all(rel_l2(same[q], ref[q]) < 1e-12 for q in SC.OUTPUTS)
