"""Cases of the per-pixel MLP backward (tests/test_gpu_pixel_mlp_backward.py runs them on the GPU; tests/test_oracle_neural.py runs every
condition on the reference alone, without one).

nns_pixel_mlp_bwd_f32 dispatches to six kernels (csrc/pixel_mlp_kernels.hip); `path_of_bwd` restates the rule:
  S1s  bf16, widths <= 32, C_in <= 4 and C_out <= 4      pixel_mlp_bwd_split_kernel<1, true>
  S1g  bf16, widths <= 32, C_in > 4 or C_out > 4         pixel_mlp_bwd_split_kernel<1, false>
  S2s  bf16, a width in 33..64, C_in, C_out <= 4         pixel_mlp_bwd_split_kernel<2, true>
  S2g  bf16, a width in 33..64, C_in > 4 or C_out > 4    pixel_mlp_bwd_split_kernel<2, false>
  Fs   float32, widths <= 32, C_in, C_out <= 4           pixel_mlp_bwd_f32_kernel<true>
  Fg   float32, widths <= 32, C_in > 4 or C_out > 4      pixel_mlp_bwd_f32_kernel<false>
followed by pixel_mlp_reduce_kernel over 4 x blocks (S1*, F*) or blocks (S2*) workspace slices, blocks = min(super-tiles of 128 pixels, 256).

The stacks, weights, biases and inputs are the forward's (pm_cases: the `sparse` and the `routing` family); the upstream gradient gy is
integers in [-2, 2].  On such data the backward is EXACT as well, and `exact_backward_reference` asserts on the float64 oracle alone why:
every delta and every layer input an MFMA takes is an integer with |v| <= 256 (bf16 holds it), and every float32 sum of a weight or bias
gradient over the pixels is below 2^24 in absolute terms, whatever its order -- so the workspace slices and the reduce kernel's sums are
exact too.  The kernels then have to equal the oracle bitwise in gx, every gW_l and every gb_l.

Sensitivity, also asserted on the reference alone (at >= 1024 pixels): in the routing family on a path's primary stack at least 3/4 of every
layer's delta channels are non-zero on some pixel and at least 2/3 of the entries of every gW_l are non-zero (the sparse family leaves most
hidden channels constant: a swapped pair of channels, lanes or k-steps between them changes nothing there); in both families on EVERY
stack gx takes at least five values, every gb_l has a non-zero entry and no two rows of the last layer's gW are equal.

Untested: the 64-bit branch of `locate` (more than 2^31 pixels: tens of GB of inputs).  And one thing these cases run but cannot see fail: the
barrier between super-tiles for an odd layer count (`if (nl & 1) __syncthreads()`) keeps the chain waves' first image stores of the next
super-tile behind the gradient waves' last image reads of this one.  With it removed from both roles every case here still passes, the
one-layer ones included: before those stores the chain waves wait for a global load, which takes several times as long as the two to eight
MFMA steps the gradient waves have left.  The barrier is what makes that ordering a guarantee and not a matter of timing.
"""
import functools

import torch

import pm_cases as PC
from oracle import neural as ON

SUPER = 128                    # pixels of a super-tile: four chain waves x 32
MAX_BLOCKS = 256               # kBwdMaxBlocks
PATHS = ('S1s', 'S1g', 'S2s', 'S2g', 'Fs', 'Fg')


def path_of_bwd(dims, bf16):
    small = dims[0] <= 4 and dims[-1] <= 4
    if not bf16:
        assert max(dims) <= 32, dims
        return 'Fs' if small else 'Fg'
    return ('S1' if max(dims) <= 32 else 'S2') + ('s' if small else 'g')


def is_bf16(path):
    return path[0] == 'S'


# path -> stacks (the forward's lists; the first one is the path's primary stack).  float32 operands: widths <= 32, i.e. the lists of S1s, S1g.
STACKS = {'S1s': PC.BF16_STACKS['A'], 'S1g': PC.BF16_STACKS['B'], 'S2s': PC.BF16_STACKS['C'], 'S2g': PC.BF16_STACKS['D'],
          'Fs': PC.BF16_STACKS['A'], 'Fg': PC.BF16_STACKS['B']}
PRIMARY = {p: STACKS[p][0][0] for p in PATHS}

# several super-tiles per workgroup: 131 074 pixels are 1025 super-tiles over 256 workgroups (four or five walks each), P is odd (super-tiles
# straddle the two items) and the last super-tile is ragged.  An odd and an even number of layers per path: the barrier between super-tiles
# exists only for an odd one.  ([2,17,31,5,4] and [3,32,32,32,3] have FOUR layers; the five-layer stack of the list is the odd one here.)
MULTI = (2, 65537)
MULTI_STACKS = {'S1s': ([4, 16, 32, 32, 16, 4], [3] + PC.W32 + [3]), 'S1g': ([5, 32, 32, 7], [17, 31, 9]),
                'S2s': ([3, 64, 33, 17, 50, 64, 40, 3], [3] + PC.W64 + [3]), 'S2g': ([40, 64, 64, 33], [5] + PC.W64 + [7])}
MULTI_STACKS['Fs'], MULTI_STACKS['Fg'] = MULTI_STACKS['S1s'], MULTI_STACKS['S1g']
# and ONE layer, where nothing but that barrier lies between a super-tile's image reads and the next one's image stores (no forward recompute).
# S2s has no such stack: one layer with at most four channels on both sides has no width above 32.  ([64, 64]: from pm_cases.F32_STACKS.)
MULTI_ONE_LAYER = {'S1s': [3, 3], 'S1g': [32, 32], 'S2g': [64, 64], 'Fs': [3, 3], 'Fg': [32, 32]}

# the reduce kernel: slice counts 4 k (S1*, F*) and k (S2*) for k super-tiles = workgroups; every count ends in a ragged super-tile.  Thread part
# q of 16 adds slices q, q + 16, ...: four at a time while q + 48 < nslices, then one at a time.  k = 13, 17: the unrolled round is entered by
# some of the 16 parts only (52, 68 slices); 16, 17 / 64, 65: at and just past a multiple of 64; 257 super-tiles: the grid's cap.
REDUCE_SUPERTILES = (1, 4, 12, 13, 16, 17, 49, 64, 65, 255, 256, 257)
# stacks whose parameter count is NO multiple of 64 (793, 846, 9866, 4238): the last workgroup of the reduce kernel is ragged too
REDUCE_STACKS = {'S1s': [2, 17, 31, 5, 4], 'S1g': [17, 31, 9], 'S2s': [3, 64, 33, 17, 50, 64, 40, 3], 'S2g': [17, 63, 47, 2]}
REDUCE_STACKS['Fs'], REDUCE_STACKS['Fg'] = REDUCE_STACKS['S1s'], REDUCE_STACKS['S1g']

# overwrite / workspace independence: each path's primary stack, one ragged count on two items
OVERWRITE = ('routing', 2, 1517)


def nparams(dims):
    return sum(ci * co + co for ci, co in zip(dims[:-1], dims[1:]))


def blocks_of(npix):
    return min((npix + SUPER - 1) // SUPER, MAX_BLOCKS)


def nslices_of(path, npix):
    return blocks_of(npix) * (1 if path[:2] == 'S2' else 4)


def reduce_pixels(k):
    return SUPER * k - 37


for _p in PATHS:
    for _d, _ in STACKS[_p]:
        assert path_of_bwd(_d, is_bf16(_p)) == _p, (_p, _d)
    assert len(MULTI_STACKS[_p][0]) % 2 == 0 and len(MULTI_STACKS[_p][1]) % 2 == 1          # odd, even number of LAYERS
    for _d in MULTI_STACKS[_p] + (REDUCE_STACKS[_p],):
        assert path_of_bwd(_d, is_bf16(_p)) == _p and any(_d == s for s, _ in STACKS[_p]), (_p, _d)
    assert nparams(REDUCE_STACKS[_p]) % 64 != 0
    assert _p == 'S2s' or (len(MULTI_ONE_LAYER[_p]) == 2 and path_of_bwd(MULTI_ONE_LAYER[_p], is_bf16(_p)) == _p)
assert (MULTI[0] * MULTI[1] + SUPER - 1) // SUPER == 1025 and MULTI[1] % 2 == 1 and (MULTI[0] * MULTI[1]) % SUPER != 0


def case_id(path, fam, dims, mb, P, why=''):
    return '%s-%s-%s-%dx%d%s' % (path, fam, PC.stack_id(dims), mb, P, '-' + why if why else '')


def exact_cases():
    """(id, path, family, dims, mb, P): each path's primary stack at every pixel count, every other stack at three of them (rotating)."""
    out = []
    for pi, path in enumerate(PATHS):
        for i, (dims, _) in enumerate(STACKS[path]):
            pix = PC.PIXELS if i == 0 else [PC.SMALL_PIXELS[(5 * i + 7 * j + 3 * pi) % len(PC.SMALL_PIXELS)] for j in range(3)]
            for mb, P, why in pix:
                for fam in ('sparse', 'routing'):
                    out.append((case_id(path, fam, dims, mb, P, why), path, fam, dims, mb, P))
    return out


def multi_cases():
    return [(case_id(path, fam, dims, *MULTI), path, fam, dims) + MULTI for path in PATHS
            for dims in MULTI_STACKS[path] + ((MULTI_ONE_LAYER[path],) if path in MULTI_ONE_LAYER else ()) for fam in ('sparse', 'routing')]


def reduce_cases():
    out = []
    for path in PATHS:
        for k in REDUCE_SUPERTILES:
            n = reduce_pixels(k)
            assert blocks_of(n) == min(k, MAX_BLOCKS) and n % SUPER != 0
            out.append((case_id(path, 'routing', REDUCE_STACKS[path], 1, n, '%d-slices' % nslices_of(path, n)), path, 'routing', REDUCE_STACKS[path], 1, n))
    return out


def overwrite_cases():
    fam, mb, P = OVERWRITE
    return [(case_id(path, fam, PRIMARY[path], mb, P), path, fam, PRIMARY[path], mb, P) for path in PATHS]


def all_exact_cases():
    return exact_cases() + multi_cases() + reduce_cases() + overwrite_cases()


# ------------------------------------------------------------------------------------------------------------------ the upstream gradient
# (family, dims) whose sums leave the bounds with gy in [-2, 2]: gy in {-1, 0, 1} there.  None does.
NARROW_GY = frozenset()


def upstream(family, dims, mb, P, seed):
    g = torch.Generator().manual_seed(424243 + 1000003 * seed + 7919 * mb + P)
    a = 1 if (family, tuple(dims)) in NARROW_GY else 2
    return torch.randint(-a, a + 1, (mb, dims[-1], P, 1), generator=g).float()


# ------------------------------------------------------------------------------------------------------------------ the exact reference
def _small_int(t):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= 256


def exact_backward_reference(family, dims, Ws, bs, x, gy, routes=None, primary=False, stats=None):
    """(gx, [gW_l], [gb_l]) of the float64 oracle for an exact case, after asserting on it that bf16 operands and float32 accumulation are exact
    in the backward too, and that the data can tell a wrong kernel from a right one.  `stats`, a dict, receives the measured margins."""
    L = len(dims) - 1
    npix = x.shape[0] * x.shape[2]
    PC.exact_reference(family, dims, Ws, bs, x, routes)                                  # the forward recompute: operands, sums, the family's rules
    assert _small_int(gy) and float(gy.abs().max()) <= 2
    Wd, bd = [w.double() for w in Ws], [b.double() for b in bs]
    gx, gWs, gbs = ON.pixel_mlp_backward(Wd, bd, x.double(), gy.double())
    ins = [x.double()]
    for l in range(L - 1):
        ins.append(torch.relu(torch.einsum('oc,bcxy->boxy', Wd[l], ins[l]) + bd[l][None, :, None, None]))
    st = dict(max_delta=0.0, max_sum=0.0, live_delta=1.0, dense_gw=1.0)
    d = gy.double()
    for l in range(L - 1, -1, -1):
        assert _small_int(d), (dims, l, float(d.abs().max()))                            # delta_l: an MFMA operand, and a summand of gb_l
        assert _small_int(ins[l]), (dims, l)                                             # a_{l-1}: the other operand of gW_l
        sw = float(torch.einsum('boxy,bcxy->oc', d.abs(), ins[l].abs()).max())
        sb = float(d.abs().sum(dim=(0, 2, 3)).max())
        assert sw < 2 ** 24 and sb < 2 ** 24, (dims, l, sw, sb)                          # gW_l, gb_l: exact in any order
        assert torch.equal(gWs[l], torch.einsum('boxy,bcxy->oc', d, ins[l])) and torch.equal(gbs[l], d.sum(dim=(0, 2, 3))), (dims, l)
        st['max_delta'], st['max_sum'] = max(st['max_delta'], float(d.abs().max())), max(st['max_sum'], sw, sb)
        live = float((d != 0).any(dim=3).any(dim=2).any(dim=0).double().mean())
        dense = float((gWs[l] != 0).double().mean())
        st['live_delta'], st['dense_gw'] = min(st['live_delta'], live), min(st['dense_gw'], dense)
        if family == 'routing' and primary and npix >= 1024:
            assert live >= 0.75, (dims, l, live)
            assert dense >= 2. / 3., (dims, l, dense)
        if npix >= 1024:
            assert bool((gbs[l] != 0).any()), (dims, l)
        assert float(torch.einsum('oc,boxy->bcxy', Wd[l].abs(), d.abs()).max()) < 2 ** 24, (dims, l)      # W_l^T delta_l: every partial sum
        d = torch.einsum('oc,boxy->bcxy', Wd[l], d)
        if l > 0:
            d = d * (ins[l] > 0).double()
    assert torch.equal(d, gx) and float(gx.abs().max()) < 2 ** 24, dims                 # gx leaves from the float32 accumulator
    if npix >= 1024:
        assert len(torch.unique(gx)) >= 5, dims
        assert torch.unique(gWs[-1], dim=0).shape[0] == dims[-1], dims                   # no two rows of the last layer's gW equal
    if stats is not None:
        stats.update(st)
    return gx, gWs, gbs


@functools.lru_cache(maxsize=None)
def build(family, dims, mb, P):
    """(Ws, bs, x, gy, (gx, gWs, gbs), stats) of an exact case; dims is a tuple.  Kept for the session: the float32 paths run the bf16 paths'
    stacks, and the CPU test builds what the GPU test runs."""
    Ws, bs, routes, seed = PC.stack(family, dims)
    x = (PC.sparse_input if family == 'sparse' else PC.routing_input)(list(dims), mb, P, seed)
    gy = upstream(family, dims, mb, P, seed)
    stats = {}
    ref = exact_backward_reference(family, list(dims), Ws, bs, x, gy, routes, primary=list(dims) in list(PRIMARY.values()), stats=stats)
    return Ws, bs, x, gy, ref, stats


# ------------------------------------------------------------------------------------------------------------------ random float data
F32_RANDOM_STACKS = [(d, s) for d, s in PC.RANDOM_STACKS if max(d) <= 32] + [([5, 32, 32, 7], (3, 37, 37))]
RANDOM_SEEDS = PC.RANDOM_SEEDS
F32_BOUND = 2e-5               # float32 operands against the unrounded float64 oracle (the bound tests/test_gpu_neural.py has held them to)


def random_case(dims, shape, seed):
    """pm_cases.random_stack and an N(0, 1) upstream gradient (float32, CPU)."""
    Ws, bs, x = PC.random_stack(dims, shape, seed)
    g = torch.Generator().manual_seed(7777 + seed)
    gy = torch.randn(shape[0], dims[-1], shape[1], shape[2], generator=g)
    return Ws, bs, x, gy


def emulated_backward(Ws, bs, x, gy, dtype):
    """ON.pixel_mlp_backward(bf16=True) on the float32 data, accumulated in `dtype`."""
    return ON.pixel_mlp_backward([w.to(dtype) for w in Ws], [b.to(dtype) for b in bs], x.to(dtype), gy.to(dtype), bf16=True)


def spread(a, b):
    """(rel-L2 of gx, largest rel-L2 of a gW_l, largest of a gb_l) between two backward results."""
    rel = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm())
    return rel(a[0], b[0]), max(rel(p, q) for p, q in zip(a[1], b[1])), max(rel(p, q) for p, q in zip(a[2], b[2]))


def row_cosines(gW, ref):
    """Cosine between each row of gW and of ref whose reference norm is above the median row norm."""
    gW, ref = gW.double(), ref.double()
    n = ref.norm(dim=1)
    keep = n > n.median() if len(n) > 1 else n > 0
    return (gW[keep] * ref[keep]).sum(dim=1) / (gW[keep].norm(dim=1) * n[keep])


# bf16 operands against the float64 oracle that rounds what the kernel rounds (oracle.neural.pixel_mlp_backward(bf16=True)).  What is left
# are operands on the other side of a bf16 rounding boundary, and ReLU masks that flip, because the kernel accumulates in float32 and the
# oracle exactly.  That effect measured on the reference alone -- rel-L2 between the emulation accumulated in float32 and in float64, CPU
# torch, pm_cases.RANDOM_STACKS, seeds 0..9, largest (smallest) value per stack; gW and gb: the worst layer --
#                          gx                   gW                   gb
#   [3,64x7,3]             1.07e-4 (2.8e-5)     1.52e-4 (3.6e-5)     1.30e-4 (2.5e-5)
#   [3,32,32,32,3]         1.77e-5 (1.7e-8)     1.12e-5 (3.5e-7)     2.35e-5 (3.0e-8)
#   [3,48,3]               3.11e-8 (1.9e-8)     4.76e-7 (3.1e-7)     7.85e-8 (2.0e-8)
#   [5,64x7,7]             1.60e-4 (2.5e-5)     2.04e-4 (1.9e-5)     1.74e-4 (2.7e-5)
#   [40,64,64,33]          4.10e-5 (3.4e-8)     4.84e-5 (1.0e-6)     2.97e-5 (5.3e-8)
#   [3,16,32,32,16,3]      5.13e-8 (6.2e-9)     3.00e-5 (2.6e-7)     1.49e-6 (3.1e-8)
# The bounds are 10 x the largest value of a column (the MFMA sums in another order than CPU torch, and flips are rare events whose count
# depends on that order).  The flips did NOT make the spread coarse: at depth 8 it is 1e-4 .. 2e-4, not the few 1e-3 that were feared, and the
# bounds stay 12 .. 40 times below the 2.4e-2 .. 7.5e-2 that separate the rounded from the unrounded oracle on the seeds used
# (tests/test_oracle_neural.py asserts both), so a kernel that does not round, or truncates, cannot pass.
RANDOM_BOUNDS = {'gx': 1.60e-3, 'gW': 2.04e-3, 'gb': 1.74e-3}
# a check per parameter row that needs no tuning: every row of a gW_l whose reference norm is above the layer's median has this cosine with the
# reference row (the float32 emulation's worst row over the stacks and seeds above: 0.9999986)
ROW_COSINE = 0.999
