"""The per-pixel MLP backward (nns_pixel_mlp_bwd_f32) pinned bit-exactly on each of its six kernels and on the reduce kernel behind them
(paths S1s, S1g, S2s, S2g, Fs, Fg of tests/pm_bwd_cases.py; the path a case takes is the first word of its id):

  * the forward's two exact input families with an integer upstream gradient (pm_bwd_cases: every operand a small integer, every sum over
    the pixels below 2^24) must equal the float64 oracle under torch.equal in gx, every gW_l and every gb_l -- each path's primary stack at
    every pixel count of pm_cases.PIXELS (P = 1, 2, 3, tiles and super-tiles that straddle items, ends on 32, 64 and 128 pixels), every
    other stack at three of them;
  * 131 074 pixels -- four or five super-tiles per workgroup, a ragged last one -- on a stack with an odd and one with an even number of
    layers per path (the barrier between super-tiles exists for odd counts only) and on a one-layer stack, twice, the two runs bitwise equal;
  * the reduce kernel at slice counts around its 4 x 16-way unrolled loop and its 16-way tail, on parameter counts that are no multiple of 64;
  * outputs and workspace pre-filled with NaN, an over-sized workspace full of 1e30: the same bits (overwritten, not accumulated; nothing
    read that was not written); a workspace one byte short: the workspace error, outputs untouched;
  * random float data: bf16 operands against the oracle that rounds what the kernel rounds, at bounds derived from the reference's own
    float32-vs-float64 spread (pm_bwd_cases.RANDOM_BOUNDS) and a cosine per gW row; float32 operands at 2e-5 against the unrounded oracle;
  * the autograd node with a non-contiguous x and a non-contiguous upstream gradient against torch autograd in float64.

Untested: the 64-bit branch of `locate` in the split kernels (more than 2^31 pixels need tens of GB).
"""
import ctypes

import pytest
import torch

import pm_bwd_cases as BC
import pm_cases as PC
from oracle import neural as ON

pytestmark = pytest.mark.gpu

EXACT, MULTI, REDUCE, OVERWRITE = BC.exact_cases(), BC.multi_cases(), BC.reduce_cases(), BC.overwrite_cases()


def bwd(Ws, bs, x, gy, bf16, **kw):
    from nns import ops
    return ops.pixel_mlp_bwd(x.cuda().contiguous(), gy.cuda().contiguous(), [w.cuda() for w in Ws], [b.cuda() for b in bs], bf16=bf16, **kw)


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_exact(got, ref, what):
    """torch.equal on gx, every gW_l, every gb_l against the float64 reference."""
    gx, gWs, gbs = got
    rgx, rgWs, rgbs = ref
    named = [('gx', gx, rgx)] + [('gW%d' % l, g, r) for l, (g, r) in enumerate(zip(gWs, rgWs))] + [('gb%d' % l, g, r) for l, (g, r) in enumerate(zip(gbs, rgbs))]
    assert len(gWs) == len(rgWs) and len(gbs) == len(rgbs)
    for name, g, r in named:
        g = g.cpu().double()
        if not torch.equal(g, r):
            bad = (g != r).nonzero()
            raise AssertionError('%s: %s differs in %d of %d entries, first at %s: %s, reference %s' % (
                what, name, len(bad), r.numel(), bad[:4].tolist(), g[tuple(bad[0])].item(), r[tuple(bad[0])].item()))


def assert_same_bits(a, b, what):
    for p, q in zip([a[0]] + list(a[1]) + list(a[2]), [b[0]] + list(b[1]) + list(b[2])):
        assert torch.equal(bits(p), bits(q)), what


def run_exact(path, family, dims, mb, P):
    assert BC.path_of_bwd(dims, BC.is_bf16(path)) == path
    Ws, bs, x, gy, ref, _ = BC.build(family, tuple(dims), mb, P)
    got = bwd(Ws, bs, x, gy, BC.is_bf16(path))
    assert_exact(got, ref, (path, family, dims, mb, P))
    return Ws, bs, x, gy, ref, got


@pytest.mark.parametrize('path,family,dims,mb,P', [c[1:] for c in EXACT], ids=[c[0] for c in EXACT])
def test_exact(path, family, dims, mb, P, gpu_device):
    run_exact(path, family, dims, mb, P)


@pytest.mark.parametrize('path,family,dims,mb,P', [c[1:] for c in MULTI], ids=[c[0] for c in MULTI])
def test_several_supertiles_per_workgroup(path, family, dims, mb, P, gpu_device):
    """1025 super-tiles over 256 workgroups, odd and even layer counts: exact, and the same bits when run again."""
    assert (mb * P + BC.SUPER - 1) // BC.SUPER > 4 * BC.MAX_BLOCKS
    Ws, bs, x, gy, ref, got = run_exact(path, family, dims, mb, P)
    assert_same_bits(bwd(Ws, bs, x, gy, BC.is_bf16(path)), got, (path, family, dims))


@pytest.mark.parametrize('path,family,dims,mb,P', [c[1:] for c in REDUCE], ids=[c[0] for c in REDUCE])
def test_reduce_slice_counts(path, family, dims, mb, P, gpu_device):
    """The workspace is full of NaN: a sum that takes in a slice no workgroup wrote, or leaves one out, cannot equal the reference."""
    Ws, bs, x, gy, ref, _ = BC.build(family, tuple(dims), mb, P)
    work = torch.full((workspace_bytes(dims) // 4,), float('nan'), device='cuda')
    assert_exact(bwd(Ws, bs, x, gy, BC.is_bf16(path), workspace=work), ref, (path, dims, BC.nslices_of(path, mb * P)))


# ------------------------------------------------------------------------------------------------------------------ overwrite, workspace
def workspace_bytes(dims):
    from nns import _lib
    n = ctypes.c_size_t(0)
    assert _lib.lib().nns_pixel_mlp_bwd_workspace((ctypes.c_int * len(dims))(*dims), len(dims) - 1, ctypes.byref(n)) == 0
    return n.value


def nan_outputs(dims, x):
    nw = sum(ci * co for ci, co in zip(dims[:-1], dims[1:]))
    return (torch.full(x.shape, float('nan'), device='cuda'), torch.full((nw,), float('nan'), device='cuda'),
            torch.full((sum(dims[1:]),), float('nan'), device='cuda'))


@pytest.mark.parametrize('path,family,dims,mb,P', [c[1:] for c in OVERWRITE], ids=[c[0] for c in OVERWRITE])
def test_outputs_overwritten_and_workspace_contents_ignored(path, family, dims, mb, P, gpu_device):
    from nns._lib import NnsError
    bf16 = BC.is_bf16(path)
    Ws, bs, x, gy, ref, _ = BC.build(family, tuple(dims), mb, P)
    nbytes = workspace_bytes(dims)
    assert nbytes == BC.MAX_BLOCKS * (1 if path[:2] == 'S2' else 4) * BC.nparams(dims) * 4
    # outputs and workspace full of NaN: every element is written before it is read or returned
    out = nan_outputs(dims, x)
    got = bwd(Ws, bs, x, gy, bf16, out=out, workspace=torch.full((nbytes // 4,), float('nan'), device='cuda'))
    assert got[0] is out[0] and got[1][0].data_ptr() == out[1].data_ptr() and got[2][0].data_ptr() == out[2].data_ptr()
    assert_exact(got, ref, (path, 'NaN'))
    assert not bool(torch.isnan(out[1]).any()) and not bool(torch.isnan(out[2]).any())
    # an over-sized workspace full of 1e30
    assert_exact(bwd(Ws, bs, x, gy, bf16, workspace=torch.full((nbytes // 4 + 1024,), 1e30, device='cuda')), ref, (path, '1e30'))
    # one byte short: the workspace error, and nothing written
    out = nan_outputs(dims, x)
    with pytest.raises(NnsError, match='workspace too small'):
        bwd(Ws, bs, x, gy, bf16, out=out, workspace=torch.zeros(nbytes - 1, dtype=torch.uint8, device='cuda'))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in out)


# ------------------------------------------------------------------------------------------------------------------ random float data
@pytest.mark.parametrize('dims,shape', PC.RANDOM_STACKS, ids=['%s-%s' % (BC.path_of_bwd(d, True), PC.stack_id(d)) for d, _ in PC.RANDOM_STACKS])
def test_random_bf16_vs_emulated_rounding(dims, shape, gpu_device):
    """bf16 operands against the float64 oracle that rounds what the kernel rounds: pm_bwd_cases.RANDOM_BOUNDS (derived there), and every gW
    row of above-median norm within ROW_COSINE of the reference row."""
    for seed in BC.RANDOM_SEEDS:
        Ws, bs, x, gy = BC.random_case(dims, shape, seed)
        ref = BC.emulated_backward(Ws, bs, x, gy, torch.float64)
        gx, gWs, gbs = bwd(Ws, bs, x, gy, True)
        got = (gx.cpu(), [g.cpu() for g in gWs], [g.cpu() for g in gbs])
        ex, ew, eb = BC.spread(got, ref)
        cos = min(float(BC.row_cosines(g, r).min()) for g, r in zip(got[1], ref[1]))
        print('pixel_mlp_bwd bf16 %s seed %d: gx %.3e (bound %.2e), gW %.3e (%.2e), gb %.3e (%.2e), worst row cosine %.7f' % (
            PC.stack_id(dims), seed, ex, BC.RANDOM_BOUNDS['gx'], ew, BC.RANDOM_BOUNDS['gW'], eb, BC.RANDOM_BOUNDS['gb'], cos))
        assert ex < BC.RANDOM_BOUNDS['gx'], (dims, seed, ex)
        assert ew < BC.RANDOM_BOUNDS['gW'], (dims, seed, ew)
        assert eb < BC.RANDOM_BOUNDS['gb'], (dims, seed, eb)
        assert cos >= BC.ROW_COSINE, (dims, seed, cos)


@pytest.mark.parametrize('dims,shape', BC.F32_RANDOM_STACKS, ids=['%s-%s' % (BC.path_of_bwd(d, False), PC.stack_id(d)) for d, _ in BC.F32_RANDOM_STACKS])
def test_random_f32_vs_oracle(dims, shape, gpu_device):
    """float32 operands against the unrounded float64 oracle: 2e-5 on gx, every gW_l and every gb_l, generic I/O included."""
    for seed in BC.RANDOM_SEEDS:
        Ws, bs, x, gy = BC.random_case(dims, shape, seed)
        ref = ON.pixel_mlp_backward([w.double() for w in Ws], [b.double() for b in bs], x.double(), gy.double())
        gx, gWs, gbs = bwd(Ws, bs, x, gy, False)
        errs = BC.spread((gx.cpu(), [g.cpu() for g in gWs], [g.cpu() for g in gbs]), ref)
        print('pixel_mlp_bwd f32 %s seed %d: gx %.3e, gW %.3e, gb %.3e (bound %.1e)' % ((PC.stack_id(dims), seed) + errs + (BC.F32_BOUND,)))
        assert max(errs) < BC.F32_BOUND, (dims, seed, errs)


# ------------------------------------------------------------------------------------------------------------------ the autograd node
@pytest.mark.parametrize('dims', [[3, 32, 32, 3], [5, 24, 7]], ids=['Fs-3.32x2.3', 'Fg-5.24.7'])
def test_autograd_node_noncontiguous(dims, gpu_device):
    """PixelMlpFn (float32 operands) fed a transposed view of x, its loss taken on a transposed view of y: the gradients of x and of every
    parameter equal torch autograd through conv2d / relu in float64 to 2e-5."""
    import torch.nn.functional as Fn
    from nns import ops
    assert BC.path_of_bwd(dims, False) == ('Fs' if dims[0] <= 4 else 'Fg')
    L, (mb, ny, nx) = len(dims) - 1, (2, 13, 9)
    Ws, bs, base = PC.random_stack(dims, (mb, ny, nx), 5)
    w = torch.randn(mb, dims[-1], ny, nx, generator=torch.Generator().manual_seed(6))
    # reference
    rW = [t.double()[:, :, None, None].requires_grad_(True) for t in Ws]
    rb = [t.double().requires_grad_(True) for t in bs]
    rbase = base.double().requires_grad_(True)
    h = rbase.transpose(2, 3)
    for l in range(L):
        h = Fn.conv2d(h, rW[l], rb[l])
        if l < L - 1:
            h = torch.relu(h)
    (h.transpose(2, 3) * w.double()).sum().backward()
    # the node
    gW = [t.cuda().requires_grad_(True) for t in Ws]
    gb = [t.cuda().requires_grad_(True) for t in bs]
    gbase = base.cuda().requires_grad_(True)
    xv = gbase.transpose(2, 3)
    assert not xv.is_contiguous()
    y = ops.PixelMlpFn.apply(xv, L, False, *gW, *gb)
    seen = []
    y.register_hook(lambda g: seen.append(g.is_contiguous()))
    (y.transpose(2, 3) * w.cuda()).sum().backward()
    assert seen == [False]                                                     # the upstream gradient did arrive non-contiguous
    rel = lambda a, b: float((a.detach().cpu().double() - b).norm() / b.norm())
    assert rel(y, h.detach()) < 1e-5
    assert rel(gbase.grad, rbase.grad) < BC.F32_BOUND
    for l in range(L):
        assert rel(gW[l].grad, rW[l].grad[:, :, 0, 0]) < BC.F32_BOUND, l
        assert rel(gb[l].grad, rb[l].grad) < BC.F32_BOUND, l
