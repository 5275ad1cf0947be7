"""The per-pixel MLP forward (nns_pixel_mlp_fwd_f32) pinned bit-exactly on each of its five kernels (paths A..E of tests/pm_cases.py; the
path a case takes is the first letter of its id):

  * two input families on which bf16 operands and float32 accumulation are exact (pm_cases: `sparse` exercises ReLU, `routing` gives every
    hidden channel a live value of its own) must equal the float64 oracle under torch.equal -- at pixel counts that isolate the division by
    P (P = 1: the 64-bit split of the four-tile kernel, P = 2 and powers of two: its multiply-shift), tiles that straddle images, and ends
    mid-tile / on a tile / on a group; once per path over more than three passes of the persistent grid (and bitwise equal to the same
    pixels in single-pass chunks);
  * the conversions: round-to-nearest-even of the inputs, of a hidden layer in every conversion unit, and of a middle layer;
  * NaN / inf in one pixel change no other pixel (the last pixel, which out-of-range lanes are clamped to, included); a guarded output buffer
    keeps every sentinel; the autograd surface returns the same bits;
  * random float data against the oracle with the kernel's operand rounding emulated (oracle.neural.pixel_mlp(bf16=True)).  The only
    legitimate difference is an operand that lands on the other side of a bf16 rounding boundary because the kernel accumulates in float32
    and the oracle exactly.  That effect, measured on the reference alone -- rel-L2 between the emulation accumulated in float32 and in
    float64, CPU torch, ten seeds, ~4500 pixels -- is at most
        [3,64x7,3] 1.8e-5   [3,32,32,32,3] 9.0e-7   [3,48,3] 4.0e-8   [5,64x7,7] 2.4e-5   [40,64,64,33] 2.5e-5   [3,16,32,32,16,3] 1.4e-5
    (as little as 2e-8 on a seed without a flip: flips are rare events whose count depends on the order of the sum, and the MFMA sums in
    another order than CPU torch, hence a margin of 10).  pm_cases.RANDOM_BOUND = 10 x 2.5e-5 = 2.5e-4, below the 6.7e-4 .. 2.3e-3 that
    separate the rounded from the unrounded oracle on the seeds used (tests/test_oracle_neural.py asserts both), so a kernel that does
    not round, or truncates, cannot pass.

Not reachable through the C ABI, hence without tests (do not look for them): pixel_mlp_fwd_kernel<true> (bf16 always takes a uniform or the
four-tile kernel), launch_fwd_uniform<2, true> (small I/O with a width above 32 takes the four-tile kernel) and the four-tile kernel's
nl == 1 branch (one layer with <= 4 channels on both sides has no width above 32).  Every listed stack fits the float32 kernel's LDS (eight
layers of width 64 need 130 of 160 KB, and eight layers is the limit), so its LDS refusal has no case either.  The npix >= 2^32 fallback of
the four-tile split needs two 17 GB buffers; P = 1 takes the same 64-bit branch.
"""
import ctypes

import numpy as np
import pytest
import torch

import pm_cases as PC
from conftest import rel_l2
from oracle import neural as ON

pytestmark = pytest.mark.gpu

EXACT = PC.exact_cases()
PATH_STACKS = [('A', [3, 32, 32, 32, 3], True), ('B', [5, 32, 32, 7], True), ('C', [3] + [64] * 7 + [3], True), ('D', [5] + [64] * 7 + [7], True),
               ('E', [40, 64, 64, 33], False)]
PATH_IDS = ['%s-%s-%s' % (p, 'bf16' if bf else 'f32', PC.stack_id(d)) for p, d, bf in PATH_STACKS]
for _p, _d, _bf in PATH_STACKS:
    assert PC.path_of(_d, _bf) == _p


def fwd(Ws, bs, x, bf16):
    from nns import ops
    return ops.pixel_mlp_fwd(x.cuda().contiguous(), [w.cuda() for w in Ws], [b.cuda() for b in bs], bf16=bf16)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('family,dims,bf16,mb,P', [c[1:] for c in EXACT], ids=[c[0] for c in EXACT])
def test_exact(family, dims, bf16, mb, P, gpu_device):
    from nns._lib import NnsError
    Ws, bs, x, ref = PC.build(family, tuple(dims), mb, P)
    if not bf16 and PC.f32_lds_bytes(dims) > PC.F32_LDS_LIMIT:
        with pytest.raises(NnsError):
            fwd(Ws, bs, x, bf16)
        return
    y = fwd(Ws, bs, x, bf16).cpu().double()
    bad = (y != ref).nonzero()
    assert torch.equal(y, ref), (len(bad), bad[:8].tolist())


@pytest.mark.parametrize('path,dims,bf16', [(p, PC.PERSISTENT_STACKS[p], p != 'E') for p in 'ABCDE'],
                         ids=['%s-%s-%dx%d-passes-of-131072' % ((p, PC.stack_id(PC.PERSISTENT_STACKS[p])) + PC.PERSISTENT) for p in 'ABCDE'])
def test_persistent_loop(path, dims, bf16, gpu_device):
    """More than three passes of the 256-workgroup grids, odd P, ragged tail: exact, and bitwise what single-pass chunks give."""
    assert PC.path_of(dims, bf16) == path
    mb, P = PC.PERSISTENT
    assert mb * P > 3 * PC.PASS_PIXELS and P % 2 and (mb * P) % 32
    Ws, bs, x, ref = PC.build('sparse', tuple(dims), mb, P)
    y = fwd(Ws, bs, x, bf16)
    assert torch.equal(y.cpu().double(), ref)
    xs = x.permute(0, 2, 1, 3).reshape(mb * P, dims[0])                                   # pixel-major
    ys = y.permute(0, 2, 1, 3).reshape(mb * P, dims[-1])
    chunk = PC.PASS_PIXELS // 2                                                           # one pass of every kernel (the float32 one: 256 x 8 x 32)
    for p0 in range(0, mb * P, chunk):
        xc = xs[p0:p0 + chunk].t().reshape(1, dims[0], -1, 1)
        yc = fwd(Ws, bs, xc, bf16)
        assert torch.equal(bits(yc.reshape(dims[-1], -1).t()), bits(ys[p0:p0 + chunk])), p0


# ------------------------------------------------------------------------------------------------------------------ rounding pins
def _f32_from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


def test_rounding_inputs_nearest_even(gpu_device):
    """[3, 3] identity, zero bias, bf16 operands: exactly x.bfloat16().float()."""
    words = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x42FE, 0x0080, 0x3EFF, 0x7F7E):       # even and odd bf16 patterns, normal
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x4000, 0xC000):
            words += [(hi << 16) | lo, ((hi | 0x8000) << 16) | lo]
    words += [0x00000000, 0x80000000, 0x7F7F0000, 0xFF7F0000,                  # +-0, the largest finite bf16
              0x00000001, 0x00008000, 0x00018000, 0x00010000, 0x007F8000, 0x807F7FFF, 0x80008001, 0x80018000]      # subnormals
    v = _f32_from_bits(words)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(v.bfloat16().float()).all())
    n = len(v)
    x = torch.stack([v, v.roll(5), v.flip(0)]).reshape(1, 3, n, 1)
    eye = [torch.eye(3)], [torch.zeros(3)]
    want = x.bfloat16().float()
    assert not torch.equal(want, x)
    y = fwd(*eye, x, True).cpu()
    assert torch.equal(y, want)
    nz = want != 0
    assert torch.equal(bits(y)[nz], bits(want)[nz])
    assert torch.equal(fwd(*eye, x, False).cpu(), x)                           # float32 operands: untouched


def _tie_inputs():
    """bf16-exact values m 2^e, m = 128..255, both signs: 3 m needs 9 or 10 bits, so 3 x is exact in float32 and rounds to bf16 at a tie (to even:
    up and down) for every fourth / second m, just off a tie never, and inexactly otherwise; then +-0."""
    m = torch.arange(128, 256, dtype=torch.float32)
    v = torch.cat([s * m * 2.0 ** e for e in (-7, 0, 9) for s in (1, -1)] + [torch.tensor([0.0, -0.0])])
    assert torch.equal(v, v.bfloat16().float())
    t = 3 * v
    up, down = t.bfloat16().float() > t, t.bfloat16().float() < t
    tie = ((3 * m) % 4 == 2) & (3 * m >= 512) | ((3 * m) % 2 == 1) & (3 * m < 512)
    assert int(tie.sum()) > 40 and int(up.sum()) > 100 and int(down.sum()) > 100
    x = torch.stack([v, v.roll(131), v.flip(0)]).reshape(1, 3, len(v), 1)
    return x


@pytest.mark.parametrize('width', [64, 32], ids=['C-3.64.3', 'A-3.32.3'])
def test_rounding_hidden_layer_every_conversion_unit(width, gpu_device):
    """3 x routed into hidden channels k, k + 1, k + 2 and the identity out: exactly relu(bf16_rne(3 x)).  k walks over the whole width, so every
    conversion unit of both tile pairs of the four-tile kernel (770 pixels: six full groups and a ragged one) carries the values once."""
    x = _tie_inputs()
    want = torch.relu((3 * x).bfloat16().float()) + 0.0
    assert not torch.equal(want, torch.relu(3 * x)) and bool((want == 0).sum() > 300)
    for k in list(range(0, width - 2, 3)) + [width - 3]:
        W1, W2 = torch.zeros(width, 3), torch.zeros(3, width)
        for c in range(3):
            W1[k + c, c], W2[c, k + c] = 3., 1.
        y = fwd([W1, W2], [torch.zeros(width), torch.zeros(3)], x, True).cpu()
        assert torch.equal(y, want), k
        assert torch.equal(bits(y), bits(want)), k                            # negatives and -0 come out as +0
        assert torch.equal(fwd([W1, W2], [torch.zeros(width), torch.zeros(3)], x, False).cpu(), torch.relu(3 * x)), k


@pytest.mark.parametrize('width', [64, 32], ids=['C-3.64.64.3', 'A-3.32.32.3'])
def test_rounding_middle_layer(width, gpu_device):
    """The same through a depth-3 stack: relu(rne(3 relu(rne(3 x)))) -- the second conversion works on an accumulator a middle layer made."""
    x = _tie_inputs()
    h1 = torch.relu((3 * x).bfloat16().float())
    want = torch.relu((3 * h1).bfloat16().float()) + 0.0
    assert not torch.equal(want, 3 * h1)
    for k in list(range(0, width - 2, 3)) + [width - 3]:
        k2 = (k + 17) % (width - 2)
        W1, W2, W3 = torch.zeros(width, 3), torch.zeros(width, width), torch.zeros(3, width)
        for c in range(3):
            W1[k + c, c], W2[k2 + c, k + c], W3[c, k2 + c] = 3., 3., 1.
        y = fwd([W1, W2, W3], [torch.zeros(width), torch.zeros(width), torch.zeros(3)], x, True).cpu()
        assert torch.equal(bits(y), bits(want)), k


# ------------------------------------------------------------------------------------------------------------------ containment, guards
@pytest.mark.parametrize('path,dims,bf16', PATH_STACKS, ids=PATH_IDS)
def test_nonfinite_pixel_stays_contained(path, dims, bf16, gpu_device):
    """NaN and +-inf in one pixel's inputs change that pixel's outputs only -- bitwise -- also when it is the LAST pixel of a count that ends
    mid-tile: the pixel the out-of-range lanes of the last tile load (clamped) and must not store."""
    mb, nx, ny = 2, 37, 41
    assert (mb * nx * ny) % 32
    Ws, bs, x = PC.random_stack(dims, (mb, nx, ny), 7)
    x = x.reshape(mb, dims[0], nx * ny, 1)
    clean = fwd(Ws, bs, x, bf16).cpu()
    assert bool(torch.isfinite(clean).all())
    poison = torch.tensor([float('nan'), float('inf'), float('-inf')])
    for b, p in ((mb - 1, nx * ny - 1), (0, 0), (0, 1000), (1, nx * ny - 26)):          # last; first; mid-tile; first lane of the last tile
        xp = x.clone()
        xp[b, :, p, 0] = poison.repeat(dims[0])[:dims[0]]
        y = fwd(Ws, bs, xp, bf16).cpu()
        keep = torch.ones(mb, nx * ny, dtype=torch.bool)
        keep[b, p] = False
        keep = keep[:, None, :, None].expand_as(y)
        assert torch.equal(bits(y)[keep], bits(clean)[keep]), (b, p)


@pytest.mark.parametrize('path,dims,bf16', PATH_STACKS, ids=PATH_IDS)
def test_output_guards_untouched(path, dims, bf16, gpu_device):
    """nns_pixel_mlp_fwd_f32 called directly with y inside a larger buffer of sentinels, ragged pixel counts: nothing outside y is written."""
    from nns import _lib
    L = _lib.lib()
    guard, sentinel = 4096, -12345.5
    for mb, P in ((3, 1517), (5, 1), (2, 33)):
        Ws, bs, x = PC.random_stack(dims, (mb, P, 1), 3)
        x = x.cuda().contiguous()
        wp = torch.cat([w.reshape(-1) for w in Ws]).cuda()
        bp = torch.cat(bs).cuda()
        n = mb * dims[-1] * P
        buf = torch.full((guard + n + guard,), sentinel, device='cuda')
        widths = (ctypes.c_int * len(dims))(*dims)
        rc = L.nns_pixel_mlp_fwd_f32(x.data_ptr(), wp.data_ptr(), bp.data_ptr(), buf.data_ptr() + 4 * guard, mb, P, widths, len(dims) - 1, int(bf16),
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.nns_last_error()
        torch.cuda.synchronize()
        out = buf.cpu()
        assert bool((out[:guard] == sentinel).all()) and bool((out[guard + n:] == sentinel).all()), (mb, P)
        assert torch.equal(bits(out[guard:guard + n].reshape(mb, dims[-1], P, 1)), bits(fwd(Ws, bs, x, bf16).cpu())), (mb, P)


def test_autograd_surface_same_bits(gpu_device):
    from nns.neural_spectral.spectral_ode import BasisFunc, PixelMLP
    from nns import ops
    torch.manual_seed(9)
    for depth, width, bf16 in ((8, 64, True), (4, 32, True), (4, 32, False)):
        m = PixelMLP(depth, width).cuda()
        for b in m.biases:
            torch.nn.init.normal_(b, std=0.3)
        x = torch.randn(2, 3, 19, 23, device='cuda')
        y = m.train_forward(x, bf16=bf16)
        assert y.requires_grad
        assert torch.equal(bits(y.detach()), bits(m(x, bf16=bf16)))
    bf = BasisFunc(19, 23).cuda()
    convs = [c for c in bf.net if isinstance(c, torch.nn.Conv2d)]
    x = torch.randn(2, 3, 19, 23, device='cuda')
    for bf16 in (False, True):
        got = bf.fused_forward(x, bf16=bf16)
        assert torch.equal(bits(got), bits(ops.pixel_mlp_fwd(x, [c.weight.detach() for c in convs], [c.bias.detach() for c in convs], bf16=bf16)))


# ------------------------------------------------------------------------------------------------------------------ random float data
@pytest.mark.parametrize('dims,shape', PC.RANDOM_STACKS, ids=['%s-%s' % (PC.path_of(d, True), PC.stack_id(d)) for d, _ in PC.RANDOM_STACKS])
def test_random_vs_emulated_rounding(dims, shape, gpu_device):
    """bf16 operands against the float64 oracle that rounds what the kernel rounds: RANDOM_BOUND (see the module docstring)."""
    for seed in PC.RANDOM_SEEDS:
        Ws, bs, x = PC.random_stack(dims, shape, seed)
        ref = PC.emulated(Ws, bs, x, torch.float64).numpy()
        err = rel_l2(fwd(Ws, bs, x, True).cpu().numpy(), ref)
        unr = rel_l2(fwd(Ws, bs, x, False).cpu().numpy(), ON.pixel_mlp([w.double() for w in Ws], [b.double() for b in bs], x.double()).numpy())
        print('pixel_mlp_fwd %s seed %d: bf16 vs emulated oracle %.3e (bound %.1e), float32 vs oracle %.3e' % (PC.stack_id(dims), seed, err, PC.RANDOM_BOUND, unr))
        assert err < PC.RANDOM_BOUND, (dims, seed, err)
        assert unr < 1e-5, (dims, seed, unr)
