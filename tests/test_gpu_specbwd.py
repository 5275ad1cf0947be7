"""The spectral residual backward (csrc/spectral_bwd_kernels.hip, nns_spec_residual_bwd_f32) pinned on each of its kernels, at the cases and
bounds of tests/specbwd_cases.py (its docstring has the dispatch rules, the reasoning behind the bounds and the figures measured on an MI355X):

  * every FFT length in both arithmetics against the float64 oracle, with a ragged last column tile or a partial last row group, and the
    all-FFT pairs; grad_u_prev / grad_v_prev bitwise; want_prev = False changes nothing else;
  * guard bands: outputs that are views into sentinel-filled buffers, the sentinel intact on both sides;
  * the `precise` policy, isotropic and anisotropic, bitwise;
  * launches in which a workgroup gets a second and a third tile: bitwise equal to the same grids in pieces small enough that none does, and
    three of the grids against the oracle;
  * the Nyquist mode analytically and a leak probe for the packed transforms;
  * ops.SpecResidualFn: upstream gradients that never arrive, non-contiguous inputs, want_prev off.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import specbwd_cases as SC
from specbwd_cases import rel_l2

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def dev(f):
    return [t.cuda() for t in f]


def run(c, f, precise=None, want_prev=True):
    from nns import ops
    return ops.spec_residual_bwd(*f, *SC.params(c), precise=c.precise if precise is None else precise, want_prev=want_prev)


def check(tag, c, got, ref, bound):
    """Prints every figure, then asserts them all."""
    errs = {q: rel_l2(g.cpu().numpy(), ref[q]) for q, g in zip(SC.OUTPUTS, got)}
    print('specbwd %s [%s]: bound %.2e  %s' % (tag, ' + '.join(SC.paths(c)), bound, '  '.join('%s %.2e' % kv for kv in errs.items())))
    assert all(torch.isfinite(g).all() for g in got[:3]), tag
    assert max(errs.values()) <= bound, (tag, bound, errs)


def check_prev(got, f, dt):
    for g, src in zip(got[3:], f[2:4]):
        assert torch.equal(bits(g), bits(SC.expected_prev(src, dt)))


# ------------------------------------------------------------------------------------------------------------------ 1. every instantiation
@pytest.mark.parametrize('c', SC.CASES, ids=[SC.case_id(c) for c in SC.CASES])
def test_backward_vs_oracle(c, gpu_device):
    f = dev(SC.fields(c))
    got = run(c, f)
    check(SC.case_id(c), c, got, SC.oracle(c), SC.bound(c))
    check_prev(got, f, SC.DT)
    gu, gv, gp, a, b = run(c, f, want_prev=False)
    assert a is None and b is None
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((gu, gv, gp), got))


# ------------------------------------------------------------------------------------------------------------------ 2. guard bands
GUARD, SENTINEL = 4096, -123456.0


@pytest.mark.parametrize('c', SC.GUARD_CASES, ids=[SC.case_id(c) for c in SC.GUARD_CASES])
def test_guard_bands(c, gpu_device):
    """The C entry point called with each output a view into a larger sentinel-filled buffer: ragged column tiles and partial row groups
    write nothing outside [0, B nx ny), and inside they write what ops.spec_residual_bwd returned."""
    from nns import _lib
    f = dev(SC.fields(c))
    want = run(c, f)
    n = c.B * c.nx * c.ny
    bufs = [torch.full((n + 2 * GUARD,), SENTINEL, device='cuda') for _ in range(5)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = [ctypes.c_void_p(b.data_ptr() + 4 * GUARD) for b in bufs]
    dt, Lx, Ly, rho, nu = SC.params(c)
    _lib.check(_lib.lib().nns_spec_residual_bwd_f32(*[ptr(t) for t in f], *out, c.B, c.nx, c.ny, dt, Lx, Ly, rho, nu, c.precise,
                                                    torch.cuda.current_stream().cuda_stream), 'nns_spec_residual_bwd_f32')
    torch.cuda.synchronize()
    for name, b, w in zip(SC.ALL_OUTPUTS, bufs, want):
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all()), name
        assert torch.equal(bits(b[GUARD:GUARD + n]), bits(w).view(-1)), name


# ------------------------------------------------------------------------------------------------------------------ 3. the precise policy
@pytest.mark.parametrize('shape', SC.POLICY_SHAPES, ids=['B%d-%dx%d' % s for s in SC.POLICY_SHAPES])
def test_precise_one_follows_the_amplification(shape, gpu_device):
    """precise = 1 is bitwise precise = 0 at amplification 4 and bitwise precise = 2 at 20 (and the two arithmetics do differ)."""
    for A, same, other in ((4.0, 0, 2), (20.0, 2, 0)):
        c = SC.Case(*shape, 1, A, False)
        f = dev(SC.fields(c))
        lib, a, b = run(c, f), run(c, f, precise=same), run(c, f, precise=other)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(lib, a)), (shape, A)
        assert not all(torch.equal(bits(x), bits(y)) for x, y in zip(lib[:3], b[:3])), (shape, A)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(run(c, f, precise=True), lib))


def test_precise_one_anisotropic_switches_both_passes(gpu_device):
    """Lx = Ly on a 64 x 1024 grid, nu such that only the y axis exceeds amplification 8: precise = 1 is bitwise precise = 2 on every output,
    so the x-pass -- whose own amplification is 0.75 -- ran in float64 too."""
    from nns import ops, _lib
    B, nx, ny = SC.ANISO_SHAPE
    L = SC.ANISO_L
    nu = SC.ANISO_AMP_Y * math.sqrt(3.0) * L / (math.pi * ny)
    f = dev(SC.fields(SC.Case(B, nx, ny, 1, 0.0, False)))
    r = {p: ops.spec_residual_bwd(*f, SC.DT, L, L, SC.RHO, nu, precise=p) for p in (0, 1, 2)}
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(r[1], r[2]))
    assert not torch.equal(bits(r[1][2]), bits(r[0][2]))
    assert _lib.lib().nns_spec_resolve_precise(1, nu, nx, L, ny, L) == 2 and _lib.lib().nns_spec_resolve_precise(1, nu, nx, L, 100, L) == 0
    ref = SC.oracle_of([t.cpu() for t in f], (SC.DT, L, L, SC.RHO, nu))
    for q, g in zip(SC.OUTPUTS, r[1]):
        assert rel_l2(g.cpu().numpy(), ref[q]) <= 1e-5, q


# ------------------------------------------------------------------------------------------------------------------ 4. more than one tile per workgroup
_MULTI_FIELDS = {}


def multi_fields(c):
    """The case's fields on the device: made once per grid size, for the largest batch of that size (grid b does not depend on the batch)."""
    key = (c.nx, c.ny)
    if key not in _MULTI_FIELDS:
        most = max(m[0].B for m in SC.MULTI if (m[0].nx, m[0].ny) == key)
        _MULTI_FIELDS[key] = dev(SC.make_fields(c.nx, c.ny, range(most)))
    return [t[:c.B] for t in _MULTI_FIELDS[key]]


@pytest.mark.parametrize('k', range(len(SC.MULTI)), ids=[SC.case_id(m[0]) for m in SC.MULTI])
def test_multi_tile_launch(k, gpu_device):
    """One call in which workgroups stride over two and three tiles (the role-split kernel's steady state, the grid-stride loops of the plain
    kernels) equals, bitwise, the same grids evaluated in consecutive pieces in which no workgroup gets a second tile; and its first, last
    and one interior grid meet the case's bound against the float64 oracle."""
    c = SC.MULTI[k][0]
    f = multi_fields(c)
    got = run(c, f)
    torch.cuda.synchronize()
    for b0, b1 in SC.chunks(c):
        part = run(c._replace(B=b1 - b0), [t[b0:b1] for t in f])
        for name, whole, piece in zip(SC.ALL_OUTPUTS, got, part):
            assert torch.equal(bits(whole[b0:b1]), bits(piece)), (name, b0, b1)
    grids = SC.compared_grids(c)
    small = SC.fields(c, grids)
    assert all(torch.equal(t[grids].cpu(), s) for t, s in zip(f, small))
    check(SC.case_id(c) + ' grids %s' % grids, c, [g[grids] for g in got], SC.oracle(c, grids), SC.bound(c, grids))
    check_prev(got, f, SC.DT)


# ------------------------------------------------------------------------------------------------------------------ 5. single modes
@pytest.mark.parametrize('N,axis,precise', SC.NYQUIST_CASES, ids=['N%d-%s-p%d' % t for t in SC.NYQUIST_CASES])
def test_nyquist_mode_analytically(N, axis, precise, gpu_device):
    """g_u = cos(N/2 2 pi s / L) along one axis, everything else zero: grad_p = -(D g_u) / rho = 0 (odd derivatives drop the Nyquist mode) and
    grad_u = g_u / dt + nu k_N^2 g_u (the Laplacian keeps it).  Then the leak probe against the oracle."""
    from nns import ops
    shape, prm, mode, k_n = SC.nyquist_setup(N, axis)
    z = torch.zeros(shape, device='cuda')
    g = mode.cuda()
    gu, gv, gp, _, _ = ops.spec_residual_bwd(z, z, g, z, z, *prm, precise=precise)
    want = (1.0 / prm[0] + prm[4] * k_n ** 2) * mode.double().numpy()
    print('specbwd nyquist N%d %s p%d: |grad_p| %.2e  grad_u %.2e  |grad_v| %.2e' % (N, axis, precise, gp.abs().max().item(),
                                                                                      rel_l2(gu.cpu().numpy(), want), gv.abs().max().item()))
    assert gp.abs().max().item() <= 1e-4
    assert rel_l2(gu.cpu().numpy(), want) <= 1e-5
    assert gv.abs().max().item() <= 1e-5 * np.abs(want).max()        # g_v = 0 shares a packed transform with g_u: rounding only
    prm, f = SC.leak_probe(N, axis)
    got = ops.spec_residual_bwd(*dev(f), *prm, precise=precise)
    ref = SC.oracle_of(f, prm)
    errs = {q: rel_l2(t.cpu().numpy(), ref[q]) for q, t in zip(SC.OUTPUTS, got)}
    print('specbwd leak probe N%d %s p%d: %s' % (N, axis, precise, '  '.join('%s %.2e' % kv for kv in errs.items())))
    assert max(errs.values()) <= 1e-5, errs


# ------------------------------------------------------------------------------------------------------------------ 6. the autograd node
@pytest.mark.parametrize('c', SC.AUTOGRAD_CASES, ids=[SC.case_id(c) for c in SC.AUTOGRAD_CASES])
def test_autograd_node(c, gpu_device, monkeypatch):
    """ops.SpecResidualFn on channel slices of a [B, 3, nx, ny] state: a loss of r_div alone (the other two upstream gradients are zeros), a
    loss of all three residuals, and u_prev / v_prev that require no gradient (want_prev off)."""
    from nns import ops
    prm = SC.params(c)
    u, v, w_u, w_v, w_d = SC.fields(c)
    state = torch.stack([u, v, w_u], dim=1).cuda().requires_grad_(True)            # p = a third field: the residual is linear in it
    prev = torch.stack([w_v, w_d], dim=1).cuda()
    calls = []
    real = ops.spec_residual_bwd

    def spy(*a, **kw):
        calls.append(a[-1] if len(a) == 12 else kw.get('want_prev', True))
        return real(*a, **kw)
    monkeypatch.setattr(ops, 'spec_residual_bwd', spy)
    weights = dev((w_u, w_v, w_d))
    zero = torch.zeros_like(u)
    for used, up_grad, tag in (((2,), False, 'r_div alone'), ((0, 1, 2), False, 'all three'), ((0, 1, 2), True, 'with u_prev, v_prev')):
        state.grad = None
        up, vp = prev[:, 0].clone().requires_grad_(up_grad), prev[:, 1].clone().requires_grad_(up_grad)
        assert not state[:, 0].is_contiguous()
        r = ops.SpecResidualFn.apply(state[:, 0], state[:, 1], state[:, 2], up, vp, *prm, c.precise)
        sum((r[i] * weights[i]).sum() for i in used).backward()
        assert calls[-1] == up_grad, tag
        g = [weights[i].cpu() if i in used else zero for i in range(3)]
        ref = SC.oracle_of((u, v) + tuple(g), prm)
        got = [state.grad[:, i] for i in range(3)]
        if used == (2,):
            assert bool((got[2] == 0).all())                                      # grad_p = -(D_x 0 + D_y 0) / rho
            bound = SC.NORTH_STAR if c.precise == 0 else min(SC.NORTH_STAR, max(10 * SC.worst(SC.vjp((u, v) + tuple(g), prm, torch.float32), ref), SC.FLOOR))
        else:
            bound = SC.bound(c)
        check('autograd %s %s' % (SC.case_id(c), tag), c, got, ref, bound)
        if up_grad:
            assert torch.equal(bits(up.grad), bits(SC.expected_prev(weights[0], prm[0]))) and torch.equal(bits(vp.grad), bits(SC.expected_prev(weights[1], prm[0])))
        else:
            assert up.grad is None and vp.grad is None
