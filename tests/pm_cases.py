"""Cases of the per-pixel MLP forward (tests/test_gpu_pixel_mlp_forward.py runs them on the GPU; tests/test_oracle_neural.py runs every
condition on the reference alone, without one).

nns_pixel_mlp_fwd_f32 dispatches to five kernels (csrc/pixel_mlp_kernels.hip, csrc/pixel_mlp_fwd4.hip); `path_of` restates the rule:
  A  bf16, widths <= 32, C_in <= 4 and C_out <= 4      pixel_mlp_fwd_uniform_kernel<1, true>
  B  bf16, widths <= 32, C_in > 4 or C_out > 4         pixel_mlp_fwd_uniform_kernel<1, false>
  C  bf16, a width in 33..64, C_in, C_out <= 4         pixel_mlp_fwd_pipe4_kernel  (four 32-pixel tiles per wave)
  D  bf16, a width in 33..64, C_in > 4 or C_out > 4    pixel_mlp_fwd_uniform_kernel<2, false>
  E  float32 operands                                  pixel_mlp_fwd_kernel<false>

Two input families on which bf16 arithmetic is EXACT: every MFMA operand is an integer with |v| <= 256 (bf16 holds 8 significant bits), every
float32 partial sum is an integer below 2^24 whatever the order of the sum, and the last layer's output is stored from the float32 accumulator
(|v| < 2^24).  `exact_reference` asserts all of that on the float64 oracle and returns it; the kernels then have to equal it bitwise.

  sparse   weights in {-1, 0, 1} with density min(1, 3 / cin), biases in {-1, 0, 1}, inputs integers in [-2, 2].  Exercises ReLU: about half
           of the hidden channels are dead.  Conditions asserted on the reference: at least 1/3 of every hidden layer's channels non-zero on
           some pixel, at least 20 % of the outputs non-zero, at least 5 distinct output values (on >= 1024 pixels; the operand bounds always).
  routing  every hidden channel reads exactly ONE channel of its layer's input (first layer: weight in {1, 2, 3}; later layers: weight 1, and -1
           on the channels o % 5 == 3), bias in {0, 1, 2, 3}, inputs integers in [1, 4]; where cout >= cin every input channel is read; the
           last layer sums disjoint groups of channels with +-1 weights.  Every channel fed by a positive weight is non-zero on EVERY pixel,
           and a channel is a function of one input channel, i.e. a table of four values: the builder picks, per channel, a table no other
           channel of the layer has.  There are only 12 cin first-layer tables (36 for three inputs), so a 64-wide layer behind three inputs
           cannot be all distinct: `check_routing` asserts that two channels of a layer coincide ONLY when every table the rules allow that
           channel is already present in the layer.
"""
import functools

import torch

from oracle import neural as ON

PASS_PIXELS = 131072          # one pass of the persistent grids: 256 workgroups x 8 waves x 64 pixels = 256 x 4 waves x 128 pixels
F32_LDS_LIMIT = 160 * 1024


def path_of(dims, bf16):
    if not bf16:
        return 'E'
    small = dims[0] <= 4 and dims[-1] <= 4
    if max(dims) <= 32:
        return 'A' if small else 'B'
    return 'C' if small else 'D'


def f32_lds_bytes(dims):
    """LDS need of the float32-operand kernel: [ot][kb][16][64] floats and 32 ot biases per layer."""
    return sum(((co + 31) // 32) * ((ci + 31) // 32) * 16 * 64 * 4 + ((co + 31) // 32) * 32 * 4 for ci, co in zip(dims[:-1], dims[1:]))


def stack_id(dims):
    out, i = [], 0
    while i < len(dims):
        j = i
        while j + 1 < len(dims) and dims[j + 1] == dims[i]:
            j += 1
        out.append('%d' % dims[i] if j == i else '%dx%d' % (dims[i], j - i + 1))
        i = j + 1
    return '.'.join(out)


# ------------------------------------------------------------------------------------------------------------------ stacks
W32, W64 = [32] * 7, [64] * 7
# path -> stacks (the first one is the path's primary stack: it runs every pixel count); value = the sparse family's seed
BF16_STACKS = {
    'A': [([3] + W32 + [3], 1), ([3, 3], 1), ([1, 32, 1], 3), ([4, 16, 32, 32, 16, 4], 1), ([2, 17, 31, 5, 4], 1)],
    'B': [([5, 32, 32, 7], 1), ([32, 32], 1), ([17, 31, 9], 1), ([3, 16, 8], 1), ([8, 16, 3], 1)],
    'C': [([3] + W64 + [3], 1), ([3, 48, 3], 1), ([4, 33, 4], 1), ([1, 64, 1], 9), ([3, 64, 33, 17, 50, 64, 40, 3], 1)],
    'D': [([5] + W64 + [7], 1), ([64] * 9, 1), ([40, 64, 64, 33], 1), ([17, 63, 47, 2], 1), ([3, 64, 64, 33], 1), ([33, 64, 3], 1)],
}
# float32 operands: the same lists ([40, 64, 64, 33] first: real data in the second input AND output tile), and [64, 64]
F32_STACKS = [([40, 64, 64, 33], 1), ([64, 64], 1)] + [sc for p in 'ABCD' for sc in BF16_STACKS[p] if sc[0] != [40, 64, 64, 33]]
ROUTING_SEED = 1
for _p, _l in BF16_STACKS.items():
    for _d, _ in _l:
        assert path_of(_d, True) == _p, (_p, _d)

# ------------------------------------------------------------------------------------------------------------------ pixel counts
# (mb, P, reason).  A tile is 32 pixels; a group is 64 pixels in the uniform kernels (A, B, D), 128 in the four-tile kernel (C), a tile in E.
PIXELS = [
    (5, 1, 'P=1:64-bit-split,mid-tile'),
    (128, 1, 'P=1,ends-on-128-group'),
    (3, 2, 'P=2,mid-tile'),
    (64, 2, 'P=2:shift-0-magic,ends-on-128-group'),
    (5, 3, 'P=3,mid-tile'),
    (32, 3, 'P=3,tiles-straddle-images,ends-on-tile-mid-group'),
    (3, 31, 'P=31,straddle,mid-tile'),
    (2, 32, 'P=32,ends-on-64-group'),
    (3, 32, 'P=32,ends-on-tile-mid-group'),
    (2, 33, 'P=33,straddle,mid-tile'),
    (3, 63, 'P=63,straddle,mid-tile'),
    (2, 64, 'P=64,ends-on-128-group'),
    (3, 64, 'P=64,ends-on-64-group-mid-128-group'),
    (2, 65, 'P=65,straddle,mid-tile'),
    (2, 127, 'P=127,straddle,mid-tile'),
    (3, 128, 'P=128,ends-on-128-group'),
    (2, 129, 'P=129,straddle,mid-tile'),
    (2, 1517, 'P=37*41,straddle,mid-tile'),
    (3, 4096, 'P=4096,ends-on-128-group'),
    (2, 65537, 'P=65537,second-pass-ragged-tail'),
]
SMALL_PIXELS = PIXELS[:-1]
PERSISTENT = (3, 131101)      # > 3 passes of 131072 pixels, odd P (tiles straddle images), ragged tail
PERSISTENT_STACKS = {'A': [3] + W32 + [3], 'B': [5, 32, 32, 7], 'C': [3] + W64 + [3], 'D': [5] + W64 + [7], 'E': [40, 64, 64, 33]}


def _seed_of(dims):
    for lst in list(BF16_STACKS.values()) + [F32_STACKS]:
        for d, s in lst:
            if d == list(dims):
                return s
    raise KeyError(dims)


def exact_cases():
    """(id, family, dims, bf16, mb, P): each path's primary stack at every pixel count, every other stack at three of them (rotating)."""
    out = []
    for bf16, groups in ((True, [BF16_STACKS[p] for p in 'ABCD']), (False, [F32_STACKS])):
        for lst in groups:
            for i, (dims, _) in enumerate(lst):
                pix = PIXELS if i == 0 else [SMALL_PIXELS[(5 * i + 7 * j + (0 if bf16 else 3)) % len(SMALL_PIXELS)] for j in range(3)]
                for mb, P, why in pix:
                    for fam in ('sparse', 'routing'):
                        out.append(('%s-%s-%s-%s-%dx%d-%s' % (path_of(dims, bf16), 'bf16' if bf16 else 'f32', fam, stack_id(dims), mb, P, why),
                                    fam, dims, bf16, mb, P))
    return out


# ------------------------------------------------------------------------------------------------------------------ sparse family
def sparse_stack(dims, seed, k=3):
    g = torch.Generator().manual_seed(seed)
    Ws, bs = [], []
    for cin, cout in zip(dims[:-1], dims[1:]):
        mask = (torch.rand(cout, cin, generator=g) < min(1.0, k / cin)).float()
        sign = (torch.randint(0, 2, (cout, cin), generator=g) * 2 - 1).float()
        Ws.append(mask * sign)
        bs.append(torch.randint(-1, 2, (cout,), generator=g).float())
    return Ws, bs


def _input(dims, mb, P, seed, lo, hi):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * mb + P)
    return torch.randint(lo, hi + 1, (mb, dims[0], P, 1), generator=g).float()


def sparse_input(dims, mb, P, seed):
    return _input(dims, mb, P, seed, -2, 2)


def routing_input(dims, mb, P, seed):
    return _input(dims, mb, P, seed, 1, 4)


# ------------------------------------------------------------------------------------------------------------------ routing family
def _const_key(c, table):
    return ('const', table[0]) if len(set(table)) == 1 else (c, table)


def _apply(func, w, b):
    c, table = func
    return c, tuple(max(w * v + b, 0) for v in table)


def _hidden_candidates(l, o, cin, cout):
    """(source channels, weights) the rules allow hidden channel o of layer l."""
    wts = (1, 2, 3) if l == 0 else ((-1,) if o % 5 == 3 else (1,))
    srcs = [o] if (cout >= cin and o < cin) else list(range(cin))
    return srcs, wts


def _reachable(funcs, l, o, cin, cout):
    """key -> (src, w, b) of every table the rules allow channel o (a channel fed by a positive weight must be non-zero everywhere)."""
    srcs, wts = _hidden_candidates(l, o, cin, cout)
    out = {}
    for s in srcs:
        for w in wts:
            for b in range(4):
                f = _apply(funcs[s], w, b)
                if w > 0 and min(f[1]) == 0:
                    continue
                out.setdefault(_const_key(*f), []).append((s, w, b))
    return out


def routing_stack(dims, seed):
    g = torch.Generator().manual_seed(seed)
    L = len(dims) - 1
    funcs = [(c, (1, 2, 3, 4)) for c in range(dims[0])]
    Ws, bs = [], []
    for l in range(L - 1):
        cin, cout = dims[l], dims[l + 1]
        W, b = torch.zeros(cout, cin), torch.zeros(cout)
        used, new = set(), []
        for o in range(cout):
            reach = _reachable(funcs, l, o, cin, cout)
            keys = sorted(reach, key=repr)
            keys = [keys[i] for i in torch.randperm(len(keys), generator=g).tolist()]
            live = [k for k in keys if k != ('const', 0)] or keys
            fresh = [k for k in live if k not in used]
            key = (fresh or live)[0]
            opts = reach[key]
            s, w, bb = opts[int(torch.randint(0, len(opts), (1,), generator=g))]
            W[o, s], b[o] = w, bb
            used.add(key)
            new.append(_apply(funcs[s], w, bb))
        funcs = new
        Ws.append(W)
        bs.append(b)
    cin, cout = dims[-2], dims[-1]
    W = torch.zeros(cout, cin)
    for c in range(cin):
        W[c % cout, c] = -1. if (c // cout) % 2 else 1.
    Ws.append(W)
    bs.append(torch.randint(0, 4, (cout,), generator=g).float())
    return Ws, bs


def check_routing(dims, Ws, bs):
    """The routing rules, re-derived from the matrices alone.  Returns per hidden layer the list of (source, weight) of its channels."""
    L = len(dims) - 1
    funcs = [(c, (1, 2, 3, 4)) for c in range(dims[0])]
    routes = []
    for l in range(L - 1):
        cin, cout = dims[l], dims[l + 1]
        W, b = Ws[l], bs[l]
        assert tuple(W.shape) == (cout, cin)
        assert bool(((W != 0).sum(dim=1) == 1).all()), (dims, l)                       # exactly one input channel each
        src = (W != 0).float().argmax(dim=1).tolist()
        wt = [int(W[o, src[o]]) for o in range(cout)]
        assert set(int(v) for v in b.tolist()) <= {0, 1, 2, 3} and bool((b == b.round()).all())
        if cout >= cin:
            assert set(src) == set(range(cin)), (dims, l)                               # every input channel is read
        new, keys = [], []
        for o in range(cout):
            assert wt[o] in _hidden_candidates(l, o, cin, cout)[1], (dims, l, o)
            f = _apply(funcs[src[o]], wt[o], int(b[o]))
            if wt[o] > 0:
                assert min(f[1]) > 0, (dims, l, o)                                     # live on every pixel
            new.append(f)
            keys.append(_const_key(*f))
        nneg = sum(1 for w in wt if w < 0)
        assert nneg == (0 if l == 0 else len([o for o in range(cout) if o % 5 == 3])) and 2 * nneg < cout, (dims, l)
        for o in range(cout):
            if keys[o] in keys[:o]:                                                     # repeats an earlier channel: only when nothing else was left to take
                assert set(_reachable(funcs, l, o, cin, cout)) - {('const', 0)} <= set(keys[:o]), (dims, l, o)
        funcs = new
        routes.append(list(zip(src, wt)))
    W = Ws[-1]
    assert bool(((W != 0).sum(dim=0) == 1).all()) and bool((W.abs() <= 1).all()), dims      # disjoint groups, every channel in one, +-1
    assert set(int(v) for v in bs[-1].tolist()) <= {0, 1, 2, 3}
    return routes


# ------------------------------------------------------------------------------------------------------------------ the exact reference
def exact_reference(family, dims, Ws, bs, x, routes=None):
    """The float64 oracle of an exact case, after asserting on it that bf16 operands and float32 accumulation are exact and that the family's
    conditions hold on this data."""
    L = len(dims) - 1
    npix = x.shape[0] * x.shape[2]
    for t in [x] + list(Ws) + list(bs):
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= 256
    if family == 'routing':
        assert float(x.min()) >= 1 and float(x.max()) <= 4
    else:
        assert float(x.abs().max()) <= 2
    h = x.double()
    for l in range(L):
        W, b = Ws[l].double(), bs[l].double()[None, :, None, None]
        assert float((torch.einsum('oc,bcxy->boxy', W.abs(), h.abs()) + b.abs()).max()) < 2 ** 24, (dims, l)     # every partial sum, any order
        z = torch.einsum('oc,bcxy->boxy', W, h) + b
        if l == L - 1:
            assert float(z.abs().max()) < 2 ** 24, dims
            break
        assert float(z.abs().max()) <= 256, (dims, l, float(z.abs().max()))
        h = torch.relu(z)
        if family == 'sparse' and npix >= 1024:
            live = (h != 0).any(dim=3).any(dim=2).any(dim=0)
            assert 3 * int(live.sum()) >= dims[l + 1], (dims, l, int(live.sum()))
        if family == 'routing':
            pos = torch.tensor([w > 0 for _, w in routes[l]])
            assert bool((h[:, pos] != 0).all()), (dims, l)                              # fed by a positive weight: non-zero on every pixel
            if 64 <= npix <= 20000 and all(len(torch.unique(x[:, c])) == 4 for c in range(dims[0])):
                # every input channel takes all four values: channels with different tables differ on some pixel
                flat = h.permute(1, 0, 2, 3).reshape(dims[l + 1], -1)
                ndist = torch.unique(flat, dim=0).shape[0]
                assert ndist == _ntables(dims, Ws, bs, l), (dims, l, ndist)
    ref = z
    assert torch.equal(ref, ON.pixel_mlp([w.double() for w in Ws], [b.double() for b in bs], x.double()))
    if family == 'sparse' and npix >= 1024:
        assert 5 * int((ref != 0).sum()) >= ref.numel(), dims
        assert len(torch.unique(ref)) >= 5, dims
    return ref


def _ntables(dims, Ws, bs, upto):
    """Distinct tables among the channels of hidden layer `upto` (check_routing has verified that this is as many as the rules allow)."""
    funcs = [(c, (1, 2, 3, 4)) for c in range(dims[0])]
    for l in range(upto + 1):
        src = (Ws[l] != 0).float().argmax(dim=1).tolist()
        funcs = [_apply(funcs[src[o]], int(Ws[l][o, src[o]]), int(bs[l][o])) for o in range(Ws[l].shape[0])]
    return len(set(_const_key(*f) for f in funcs))


@functools.lru_cache(maxsize=None)
def stack(family, dims):
    """(Ws, bs, routes, seed) of a family's stack; dims is a tuple."""
    dims = list(dims)
    if family == 'sparse':
        seed = _seed_of(dims)
        return sparse_stack(dims, seed) + (None, seed)
    Ws, bs = routing_stack(dims, ROUTING_SEED)
    return Ws, bs, check_routing(dims, Ws, bs), ROUTING_SEED


@functools.lru_cache(maxsize=8)
def build(family, dims, mb, P):
    """(Ws, bs, x, ref) of an exact case; dims is a tuple."""
    Ws, bs, routes, seed = stack(family, dims)
    x = (sparse_input if family == 'sparse' else routing_input)(list(dims), mb, P, seed)
    return Ws, bs, x, exact_reference(family, list(dims), Ws, bs, x, routes)


# ------------------------------------------------------------------------------------------------------------------ random float stacks
RANDOM_STACKS = [([3] + W64 + [3], (3, 37, 41)), ([3, 32, 32, 32, 3], (2, 45, 47)), ([3, 48, 3], (5, 9, 91)), ([5] + W64 + [7], (3, 37, 37)),
                 ([40, 64, 64, 33], (2, 61, 33)), ([3, 16, 32, 32, 16, 3], (3, 29, 47))]


def random_stack(dims, shape, seed):
    """kaiming-uniform weights as torch initialises a Conv2d (a = sqrt(5): U(-1, 1) / sqrt(cin)), N(0, 0.3) biases, N(0, 1) inputs (float32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    Ws = [(torch.rand(co, ci, generator=g) * 2 - 1) / ci ** 0.5 for ci, co in zip(dims[:-1], dims[1:])]
    bs = [0.3 * torch.randn(co, generator=g) for co in dims[1:]]
    x = torch.randn(shape[0], dims[0], shape[1], shape[2], generator=g)
    return Ws, bs, x


def emulated(Ws, bs, x, dtype):
    """ON.pixel_mlp(bf16=True) on the float32 data, accumulated in `dtype`."""
    return ON.pixel_mlp([w.to(dtype) for w in Ws], [b.to(dtype) for b in bs], x.to(dtype), bf16=True)


RANDOM_SEEDS = (1, 2)
# 10 x the largest rel-L2 between the emulation accumulated in float32 and in float64 (CPU torch, RANDOM_STACKS, seeds 0..9: 2.5e-5)
RANDOM_BOUND = 2.5e-4
