"""The neural oracle (oracle/neural.py) vs golden vectors captured from the reference's PDEFunc /
ANODE integrators / BasisFunc (float32 in the reference; the oracle is run in float32 here for a
tight comparison and in float64 to bound the fp32 rounding of the reference itself)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
from oracle import neural as ON

G = load_golden('neural_spectral.npz')


def T(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype)


def mlp_from(prefix, dtype=torch.float32, req=False):
    ps = [T(G[prefix + 'net.%d.%s' % (i, w)], dtype) for i in (0, 2, 4) for w in ('weight', 'bias')]
    if req:
        for p in ps:
            p.requires_grad_(True)
    return tuple(ps)


@pytest.mark.parametrize('method', ['Euler', 'RK2', 'RK4'])
def test_integrators(method):
    out = ON.integrate(mlp_from('ode_'), T(G['ode_z0']), 7, method)
    assert out.shape == (7, 3, 12)
    assert rel_l2(out.numpy(), G['ode_' + method]) < 2e-6
    out64 = ON.integrate(mlp_from('ode_', torch.float64), T(G['ode_z0'], torch.float64), 7, method)
    assert rel_l2(out64.numpy(), G['ode_' + method]) < 2e-6


@pytest.mark.parametrize('mb', [1, 3])
def test_spectral_ode_forward_loss_grads(mb):
    K = 4
    init = T(G['s1_param_init_coeffs']).requires_grad_(True)
    mlp = mlp_from('s1_param_basis_coeffs.', req=True)
    basis = torch.stack([T(G['s1_param_basis_fns.%d' % k]) for k in range(K)]).requires_grad_(True)
    obs = T(G['s1_mb%d_obs' % mb])
    pred, _ = ON.pde_forward(init, mlp, basis, mb, obs.shape[0])
    assert rel_l2(pred.detach().numpy(), G['s1_mb%d_pred' % mb]) < 2e-6
    loss = ON.loss_fn(pred, obs)
    assert abs(loss.item() - float(G['s1_mb%d_loss' % mb])) < 1e-5 * float(G['s1_mb%d_loss' % mb])
    loss.backward()
    pre = 's1_mb%d_grad_' % mb
    assert rel_l2(init.grad.numpy(), G[pre + 'init_coeffs']) < 1e-4
    for i, idx in enumerate((0, 2, 4)):
        assert rel_l2(mlp[2 * i].grad.numpy(), G[pre + 'basis_coeffs.net.%d.weight' % idx]) < 1e-4
        assert rel_l2(mlp[2 * i + 1].grad.numpy(), G[pre + 'basis_coeffs.net.%d.bias' % idx]) < 1e-4
    for k in range(K):
        assert rel_l2(basis.grad[k].numpy(), G[pre + 'basis_fns.%d' % k]) < 1e-5


@pytest.mark.parametrize('mb', [1, 3])
def test_spectral_ode2_forward_loss_grads(mb):
    K = 4
    inits = [T(G['s2_param_%s_init_coeffs' % c]).requires_grad_(True) for c in 'uvp']
    mlps = [mlp_from('s2_param_%s_basis_coeffs.' % c, req=True) for c in 'uvp']
    bases = [torch.stack([T(G['s2_param_%s_basis_fns.%d' % (c, k)]) for k in range(K)]).requires_grad_(True)
             for c in 'uvp']
    obs = T(G['s2_mb%d_obs' % mb])
    pred = ON.pde2_forward(inits, mlps, bases, mb, obs.shape[0])
    assert rel_l2(pred.detach().numpy(), G['s2_mb%d_pred' % mb]) < 2e-6
    loss = ON.loss_fn(pred, obs)
    loss.backward()
    pre = 's2_mb%d_grad_' % mb
    for ci, c in enumerate('uvp'):
        assert rel_l2(inits[ci].grad.numpy(), G[pre + '%s_init_coeffs' % c]) < 1e-4
        for k in range(K):
            assert rel_l2(bases[ci].grad[k].numpy(), G[pre + '%s_basis_fns.%d' % (c, k)]) < 1e-5
        assert rel_l2(mlps[ci][2].grad.numpy(), G[pre + '%s_basis_coeffs.net.2.weight' % c]) < 1e-4


def test_diversity_penalty():
    basis = torch.stack([T(G['s1_param_basis_fns.%d' % k]) for k in range(4)])
    assert abs(ON.diversity_penalty(basis).item() - float(G['s1_diversity_penalty'])) < 1e-6 * float(
        G['s1_diversity_penalty'])


def test_pixel_mlp_basisfunc():
    idx = (0, 2, 4, 6, 8)
    Ws = [T(G['bf_param_net.%d.weight' % i])[:, :, 0, 0].clone().requires_grad_(True) for i in idx]
    bs = [T(G['bf_param_net.%d.bias' % i]).requires_grad_(True) for i in idx]
    x = T(G['bf_in']).requires_grad_(True)
    y = ON.pixel_mlp(Ws, bs, x)
    assert rel_l2(y.detach().numpy(), G['bf_out']) < 2e-6
    (y * T(G['bf_w'])).sum().backward()
    assert rel_l2(x.grad.numpy(), G['bf_grad_in']) < 1e-5
    for W, b, i in zip(Ws, bs, idx):
        assert rel_l2(W.grad.numpy(), G['bf_grad_net.%d.weight' % i][:, :, 0, 0]) < 1e-5
        assert rel_l2(b.grad.numpy(), G['bf_grad_net.%d.bias' % i]) < 1e-5


def test_pixel_mlp_backward_matches_autograd():
    """The hand-written reverse mode used as the checker of the fused HIP backward equals torch.autograd (float64)."""
    torch.manual_seed(3)
    dims = [3, 16, 24, 5]
    Ws = [torch.randn(dims[i + 1], dims[i], dtype=torch.float64, requires_grad=True) for i in range(3)]
    bs = [torch.randn(dims[i + 1], dtype=torch.float64, requires_grad=True) for i in range(3)]
    x = torch.randn(2, 3, 5, 7, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(2, 5, 5, 7, dtype=torch.float64)
    y = ON.pixel_mlp(Ws, bs, x)
    y.backward(gy)
    gx, gWs, gbs = ON.pixel_mlp_backward([w.detach() for w in Ws], [b.detach() for b in bs], x.detach(), gy)
    assert torch.allclose(gx, x.grad, rtol=1e-12, atol=1e-12)
    for l in range(3):
        assert torch.allclose(gWs[l], Ws[l].grad, rtol=1e-12, atol=1e-12)
        assert torch.allclose(gbs[l], bs[l].grad, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# pixel_mlp(bf16=True): the forward kernels' operand rounding emulated, and the exact input families of tests/pm_cases.py
# (what tests/test_gpu_pixel_mlp_forward.py holds the HIP kernels to), on the reference alone.
def _pixel_mlp_unrounded(weights, biases, grid):
    """pixel_mlp as it was before it learnt to round."""
    h = grid
    for l, (W, b) in enumerate(zip(weights, biases)):
        h = torch.einsum('oc,bcxy->boxy', W, h) + b[None, :, None, None]
        if l < len(weights) - 1:
            h = torch.relu(h)
    return h


def test_pixel_mlp_default_is_unrounded():
    import pm_cases as PC
    for dtype in (torch.float32, torch.float64):
        for dims, shape in PC.RANDOM_STACKS[:3]:
            Ws, bs, x = PC.random_stack(dims, (1, 9, 7), 4)
            args = [w.to(dtype) for w in Ws], [b.to(dtype) for b in bs], x.to(dtype)
            assert torch.equal(ON.pixel_mlp(*args), _pixel_mlp_unrounded(*args))
            assert torch.equal(ON.pixel_mlp(*args, bf16=False), _pixel_mlp_unrounded(*args))


def test_pixel_mlp_bf16_rounds_what_the_backward_oracle_rounds(monkeypatch):
    """The layer inputs pixel_mlp(bf16=True) multiplies are the `ins` pixel_mlp_backward(bf16=True) builds, and with gy = 1 on one output its
    bias gradient of the last layer confirms that both see the same forward."""
    import pm_cases as PC
    dims, shape = [5, 64, 33, 7], (2, 6, 5)
    Ws, bs, x = PC.random_stack(dims, shape, 2)
    Ws, bs, x = [w.double() for w in Ws], [b.double() for b in bs], x.double()
    seen = {}
    real = torch.einsum

    def spy(eq, a, b):
        seen.setdefault(eq, []).append((a, b))
        return real(eq, a, b)
    monkeypatch.setattr(torch, 'einsum', spy)
    y = ON.pixel_mlp(Ws, bs, x, bf16=True)
    fwd = seen.pop('oc,bcxy->boxy')
    seen.clear()
    ON.pixel_mlp_backward(Ws, bs, x, torch.ones_like(y), bf16=True)
    bwd = seen['oc,bcxy->boxy']
    monkeypatch.undo()
    assert len(fwd) == len(bwd) == 3
    for (Wf, hf), (Wb, hb) in zip(fwd, bwd):
        assert torch.equal(Wf, Wb) and torch.equal(hf, hb)
        assert torch.equal(hf, hf.float().bfloat16().double()) and torch.equal(Wf, Wf.float().bfloat16().double())     # they ARE bf16 values
    assert not torch.equal(y, y.float().bfloat16().double())                                # the last layer's output is not rounded
    assert not torch.equal(y, ON.pixel_mlp(Ws, bs, x))


def test_pixel_mlp_exact_families_hold_their_conditions():
    """Every exact case the GPU test runs: the operand bounds, the liveness conditions and the routing rules hold on the float64 oracle
    (pm_cases.build asserts them), and rounding the operands to bf16 changes nothing -- bitwise."""
    import pm_cases as PC
    done = set()
    for cid, fam, dims, bf16, mb, P in PC.exact_cases():
        if (fam, tuple(dims), mb, P) in done or mb * P > 20000:
            continue
        done.add((fam, tuple(dims), mb, P))
        Ws, bs, x, ref = PC.build(fam, tuple(dims), mb, P)
        args = [w.double() for w in Ws], [b.double() for b in bs], x.double()
        assert torch.equal(ON.pixel_mlp(*args, bf16=True), ref), cid
        assert torch.equal(ON.pixel_mlp(*[[t.float() for t in a] if isinstance(a, list) else a.float() for a in args], bf16=True).double(), ref), cid
    # every stack on 4096 pixels, where the liveness conditions are asserted whatever the case's own pixel count
    for dims in sorted(set(tuple(d) for _, _, d, _, _, _ in PC.exact_cases())):
        for fam in ('sparse', 'routing'):
            Ws, bs, x, ref = PC.build(fam, dims, 1, 4096)
            assert torch.equal(ON.pixel_mlp([w.double() for w in Ws], [b.double() for b in bs], x.double(), bf16=True), ref), (fam, dims)


def test_pixel_mlp_exact_cases_reach_every_path():
    """Each dispatch path at a pixel count that ends mid-tile, on a tile boundary and on a group boundary (64 pixels for the uniform
    kernels, 128 for the four-tile kernel, the 32-pixel tile itself for the float32 kernel), all spanning at least two images."""
    import pm_cases as PC
    ends = {p: set() for p in 'ABCDE'}
    for cid, fam, dims, bf16, mb, P in PC.exact_cases():
        path = PC.path_of(dims, bf16)
        assert cid.startswith(path + '-') and mb >= 2
        n, grp = mb * P, {'C': 128, 'E': 32}.get(path, 64)
        ends[path].add('mid-tile' if n % 32 else ('group' if n % grp == 0 else 'tile'))
        if not bf16:
            assert PC.f32_lds_bytes(dims) <= PC.F32_LDS_LIMIT            # (eight layers of width 64 need 130 KB: every listed stack fits)
    for p in 'ABCD':
        assert ends[p] == {'mid-tile', 'tile', 'group'}, (p, ends[p])
    assert ends['E'] == {'mid-tile', 'group'}
    assert PC.f32_lds_bytes([64] * 9) == 8 * (4 * 16 * 64 * 4 + 256)


def test_pixel_mlp_bf16_rounding_is_visible_on_random_stacks():
    """On the random float stacks of the GPU test the rounded and the unrounded oracle differ by 5e-4 .. 2e-2 rel-L2 (measured 6.7e-4 ..
    2.3e-3 on these seeds): above RANDOM_BOUND, so a kernel that does not round cannot pass there.  And the bound itself: ten times the
    largest rel-L2 between the emulation accumulated in float32 and in float64 (re-measured here on the GPU test's seeds; the docstring of
    tests/test_gpu_pixel_mlp_forward.py has the ten-seed figures)."""
    import pm_cases as PC
    assert PC.RANDOM_BOUND <= 1e-3
    for dims, shape in PC.RANDOM_STACKS:
        for seed in PC.RANDOM_SEEDS:
            Ws, bs, x = PC.random_stack(dims, shape, seed)
            e64 = PC.emulated(Ws, bs, x, torch.float64).numpy()
            un = ON.pixel_mlp([w.double() for w in Ws], [b.double() for b in bs], x.double()).numpy()
            assert 5e-4 < rel_l2(e64, un) < 2e-2, (dims, seed, rel_l2(e64, un))
            assert rel_l2(e64, un) > 2 * PC.RANDOM_BOUND
            assert 10 * rel_l2(PC.emulated(Ws, bs, x, torch.float32).numpy(), e64) <= PC.RANDOM_BOUND, (dims, seed)


# ---------------------------------------------------------------------------------------------------------------------
# The fused ODEFunc integrator's cases (tests/ode_cases.py; tests/test_gpu_ode_mlp.py holds the HIP kernels to them), on the reference alone.
def test_step_is_what_integrate_takes():
    """integrate is Nt calls of step with dt = 1 / Nt, bitwise; step takes a free dt."""
    import ode_cases as OC
    for method in OC.METHODS:
        mlp, z0, _ = OC.inputs(17, 33, 5)
        mlp, y = [p.double() for p in mlp], z0.double()
        traj = ON.integrate(mlp, y, 5, method)
        for n in range(5):
            y = ON.step(mlp, y, 1. / 5., method)
            assert torch.equal(y, traj[n])
        f = ON.odefunc(mlp, y)
        assert torch.equal(ON.step(mlp, y, OC.STEP_DT, 'Euler'), y + OC.STEP_DT * f)
    with pytest.raises(ValueError):
        ON.step(mlp, y, 0.1, 'RK3')


def test_ode_cases_hold_their_conditions():
    """Every case and scheme of the GPU test: half of the ReLU units live and half of the ELU pre-activations negative at the first stage, and
    the float32 oracle within 1e-6 of the float64 one on the trajectory and all seven gradients (so that 10 x that is a bound a float32
    kernel can be held to, and no ReLU kink decides the comparison)."""
    import ode_cases as OC
    assert [c[:3] for c in OC.CASES] == [(1, 1, 1), (1, 17, 2), (2, 16, 3), (15, 15, 4), (16, 1, 1), (17, 33, 5), (31, 17, 3), (32, 16, 2), (32, 49, 4),
                                         (30, 5, 60)]
    for K, mb, Nt in OC.SHAPES:
        live, neg = OC.first_stage_shares(K, mb, Nt)
        print('ode case %s: live ReLU %.3f, negative ELU %.3f' % (OC.case_id(K, mb, Nt), live, neg))
        assert 0.3 <= live <= 0.7 and 0.3 <= neg <= 0.7, (K, mb, Nt, live, neg)
        (W0, b0, W1, b1, W2, b2), z0, w = OC.inputs(K, mb, Nt)
        assert W0.shape == (128, K) and W1.shape == (128, 128) and W2.shape == (K, 128) and z0.shape == (mb, K) and w.shape == (Nt, mb, K)
        for method in OC.METHODS:
            e = OC.e32(K, mb, Nt, method)
            print('ode case %s: e32 %.2e, bound %.2e' % (OC.case_id(K, mb, Nt, method), e, OC.bound(K, mb, Nt, method)))
            assert 0 < e <= OC.E32_LIMIT, (K, mb, Nt, method, e)
            assert OC.bound(K, mb, Nt, method) == max(10 * e, 2e-6)
            ref = OC.oracle(K, mb, Nt, method)
            assert ref['traj'].shape == (Nt, mb, K) and all(np.abs(ref[q]).max() > 0 for q in OC.QUANTITIES)
    for K, rows, method in OC.STEP_CASES:
        e = OC.step_e32(K, rows, method)
        assert 0 < e <= OC.E32_LIMIT, (K, rows, method, e)
        assert OC.step_bound(K, rows, method) == max(10 * e, 2e-6)


def test_ode_bound_rejects_wrong_oracles():
    """The bound of every case, applied to three deliberately wrong float64 oracles, fails by at least 100 x on every quantity the mutation
    acts on: RK4 weights 1/6 and 1/3 exchanged, ELU derivative taken as 1 for z < 0, row mb - 1 left out of the parameter gradients."""
    import ode_cases as OC
    acted = {m: 0 for m in OC.MUTATIONS}
    for K, mb, Nt, method in OC.CASE_METHODS:
        ref = OC.oracle(K, mb, Nt, method)
        same = OC.mutant(None, K, mb, Nt, method)
        assert all(np.array_equal(same[q], ref[q]) for q in OC.QUANTITIES)          # the mutants' integrator, unmutated, IS the oracle
        for mutation in OC.MUTATIONS:
            if not OC.mutation_acts(mutation, K, mb, Nt, method):
                continue
            acted[mutation] += 1
            bad = OC.mutant(mutation, K, mb, Nt, method)
            hit = OC.mutation_quantities(mutation, Nt, method)
            for q in OC.QUANTITIES:
                err = rel_l2(bad[q], ref[q])
                if q in hit:
                    assert err >= 100 * OC.bound(K, mb, Nt, method), (mutation, K, mb, Nt, method, q, err)
                elif mutation != 'rk4_weights':
                    assert err < 1e-14, (mutation, K, mb, Nt, method, q, err)        # and nothing else moves (float64 rounding: the batch is split)
    assert acted == {'rk4_weights': 10, 'elu_grad': 30, 'drop_row': 24}


def test_elu_points_cover_what_elu1_branches_on():
    import ode_cases as OC
    z = OC.elu_points().numpy().ravel()
    assert z.dtype == np.float32 and len(z) == 2048 and z.min() == -110 and z.max() == 2
    split = np.float32(OC.ELU_SPLIT)
    for edge in (np.float32(0), split):
        for side in (-np.inf, np.inf):
            assert np.nextafter(edge, np.float32(side)) in z
        assert edge in z
    assert ((z > split - 0.01) & (z < split + 0.01)).sum() > 500 and (np.abs(z) < 0.005).sum() > 400
    assert (z <= OC.ELU_EXACT_MINUS_ONE).sum() > 100 and ((z < -17.4) & (z > OC.ELU_EXACT_MINUS_ONE)).sum() >= 1
    assert np.all(np.float32(OC.elu_expected(z[z <= OC.ELU_EXACT_MINUS_ONE])) == -1)
    assert (z > 0).sum() > 300 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    # a float32 expm1 is within the read-out's bound of the float64 one; elu taken as z everywhere is not
    rel, neg = OC.elu_errors(z, np.where(z > 0, z, np.expm1(z)).astype(np.float32))
    assert rel.max() < 2.4e-7                       # two float32 roundings
    lin = np.where(z > OC.ELU_EXACT_MINUS_ONE, np.where(z > -1e-3, z, np.expm1(z.astype(np.float64))), -1).astype(np.float32)      # first order near 0
    assert OC.elu_errors(z, lin)[0].max() > 100 * OC.ELU_REL


# ---------------------------------------------------------------------------------------------------------------------
# The per-pixel MLP backward's cases (tests/pm_bwd_cases.py; tests/test_gpu_pixel_mlp_backward.py holds the HIP kernels to them), on the
# reference alone.
def test_pixel_mlp_bwd_cases_reach_every_path():
    """path_of_bwd puts every listed stack on the path it is listed under; each path has its primary stack at every pixel count in both
    families, an odd and an even layer count at 131 074 pixels, and the reduce kernel's slice counts."""
    import pm_bwd_cases as BC
    import pm_cases as PC
    for path in BC.PATHS:
        bf16 = path[0] == 'S'
        for dims in [d for d, _ in BC.STACKS[path]] + list(BC.MULTI_STACKS[path]) + [BC.REDUCE_STACKS[path]] + [d for p, d in BC.MULTI_ONE_LAYER.items() if p == path]:
            assert BC.path_of_bwd(dims, bf16) == path, (path, dims)
            assert (max(dims) <= 32) == (path[:2] in ('S1', 'Fs', 'Fg')) and (dims[0] <= 4 and dims[-1] <= 4) == (path[-1] == 's')
        mine = [c for c in BC.exact_cases() if c[1] == path]
        assert set((f, mb, P) for _, _, f, d, mb, P in mine if d == BC.PRIMARY[path]) == set((f, mb, P) for f in ('sparse', 'routing') for mb, P, _ in PC.PIXELS)
        assert all(sum(1 for c in mine if c[3] == d) == 6 for d, _ in BC.STACKS[path][1:])
        odd, even = BC.MULTI_STACKS[path]
        assert (len(odd) - 1) % 2 == 1 and (len(even) - 1) % 2 == 0
        assert [len(c[3]) for c in BC.multi_cases() if c[1] == path].count(2) == (0 if path == 'S2s' else 2)      # one layer, both families
        slices = [BC.nslices_of(path, P) for _, p, _, _, _, P in BC.reduce_cases() if p == path]
        unit = 1 if path[:2] == 'S2' else 4
        assert slices == [unit * min(k, 256) for k in (1, 4, 12, 13, 16, 17, 49, 64, 65, 255, 256, 257)]
        assert BC.nparams(BC.REDUCE_STACKS[path]) % 64
    assert sorted(BC.path_of_bwd(d, True) for d, _ in PC.RANDOM_STACKS) == ['S1s', 'S1s', 'S2g', 'S2g', 'S2s', 'S2s']
    assert sorted(BC.path_of_bwd(d, False) for d, _ in BC.F32_RANDOM_STACKS) == ['Fg', 'Fs', 'Fs']
    ids = [c[0] for c in BC.all_exact_cases()]
    assert len(set(ids)) == len(ids)


def test_pixel_mlp_bwd_exact_cases_hold_their_conditions():
    """Every exact case the GPU test runs -- pixel-count edges, 131 074 pixels, reduce slice counts, overwrite -- passes the conditions of
    pm_bwd_cases.exact_backward_reference: building the reference is the test (one build per stack, family and pixel count).  The margins:
    no delta above 92, no absolute sum above 2^24 / 3, and the routing family's primary stacks keep 3/4 of the delta channels and 2/3 of
    every gW_l's entries alive."""
    import pm_bwd_cases as BC
    done, worst = set(), dict(max_delta=0.0, max_sum=0.0)
    for cid, path, fam, dims, mb, P in BC.all_exact_cases():
        key = (fam, tuple(dims), mb, P)
        if key in done:
            continue
        done.add(key)
        Ws, bs, x, gy, (gx, gWs, gbs), st = BC.build(*key)
        assert gx.shape == x.shape and [g.shape for g in gWs] == [w.shape for w in Ws] and gx.dtype == torch.float64, cid
        assert float(gy.abs().max()) <= 2
        worst = {k: max(v, st[k]) for k, v in worst.items()}
        if fam == 'routing' and dims in BC.PRIMARY.values() and mb * P >= 1024:
            assert st['live_delta'] >= 0.75 and st['dense_gw'] >= 2. / 3., (cid, st)
        # and rounding the operands to bf16 changes nothing, bitwise
        if mb * P <= 20000:
            e = ON.pixel_mlp_backward([w.double() for w in Ws], [b.double() for b in bs], x.double(), gy.double(), bf16=True)
            assert torch.equal(e[0], gx) and all(torch.equal(a, b) for a, b in zip(e[1] + e[2], gWs + gbs)), cid
    print('pixel_mlp_bwd exact cases: %d references, largest |delta| %g, largest absolute sum %g' % (len(done), worst['max_delta'], worst['max_sum']))
    assert worst['max_delta'] <= 92 and 3 * worst['max_sum'] < 2 ** 24
    assert not BC.NARROW_GY


def test_pixel_mlp_bwd_reference_rejects_cases_that_are_not_exact():
    """The conditions bite: an upstream gradient of 300 (above what bf16 holds exactly), a half (no integer), a 3 (outside [-2, 2]) and an
    all-zero one (dead deltas) are refused."""
    import pm_bwd_cases as BC
    import pm_cases as PC
    dims = [5, 32, 32, 7]
    Ws, bs, routes, seed = PC.stack('routing', tuple(dims))
    x = PC.routing_input(dims, 2, 1517, seed)
    gy = BC.upstream('routing', dims, 2, 1517, seed)
    BC.exact_backward_reference('routing', dims, Ws, bs, x, gy, routes, primary=True)
    for bad in (300., 0.5, 3.):
        g2 = gy.clone()
        g2[1, 3, 700, 0] = bad
        with pytest.raises(AssertionError):
            BC.exact_backward_reference('routing', dims, Ws, bs, x, g2, routes, primary=True)
    with pytest.raises(AssertionError):
        BC.exact_backward_reference('routing', dims, Ws, bs, x, torch.zeros_like(gy), routes, primary=True)


def test_pixel_mlp_backward_matches_autograd_on_generic_stacks():
    """oracle.neural.pixel_mlp_backward equals torch autograd in float64 on two of the backward test's stacks (generic I/O, widths that
    are no multiple of 16)."""
    import pm_bwd_cases as BC
    for dims, shape in (([5, 32, 32, 7], (2, 9, 7)), ([3, 64, 33, 17, 50, 64, 40, 3], (2, 5, 11))):
        Ws, bs, x, gy = [[u.double().requires_grad_(True) for u in t] if isinstance(t, list) else t.double() for t in BC.random_case(dims, shape, 3)]
        x.requires_grad_(True)
        ON.pixel_mlp(Ws, bs, x).backward(gy)
        gx, gWs, gbs = ON.pixel_mlp_backward([w.detach() for w in Ws], [b.detach() for b in bs], x.detach(), gy)
        assert torch.allclose(gx, x.grad, rtol=1e-12, atol=1e-12)
        for l in range(len(Ws)):
            assert torch.allclose(gWs[l], Ws[l].grad, rtol=1e-12, atol=1e-12) and torch.allclose(gbs[l], bs[l].grad, rtol=1e-12, atol=1e-12)
            assert float(Ws[l].grad.abs().max()) > 0


def test_pixel_mlp_bwd_random_bounds_come_from_the_reference():
    """RANDOM_BOUNDS are ten times the reference's own float32-vs-float64 spread (re-measured here on the GPU test's seeds; pm_bwd_cases has the
    ten-seed figures), and at least 10 x below what separates the rounded from the unrounded oracle there."""
    import pm_bwd_cases as BC
    import pm_cases as PC
    assert BC.RANDOM_BOUNDS == {'gx': 1.60e-3, 'gW': 2.04e-3, 'gb': 1.74e-3} and BC.ROW_COSINE == 0.999 and BC.F32_BOUND == 2e-5
    for dims, shape in PC.RANDOM_STACKS:
        for seed in BC.RANDOM_SEEDS:
            Ws, bs, x, gy = BC.random_case(dims, shape, seed)
            e64 = BC.emulated_backward(Ws, bs, x, gy, torch.float64)
            e32 = BC.emulated_backward(Ws, bs, x, gy, torch.float32)
            un = ON.pixel_mlp_backward([w.double() for w in Ws], [b.double() for b in bs], x.double(), gy.double())
            for name, own, gap in zip(('gx', 'gW', 'gb'), BC.spread(e32, e64), BC.spread(e64, un)):
                assert 10 * own <= BC.RANDOM_BOUNDS[name], (dims, seed, name, own)
                assert gap > 10 * BC.RANDOM_BOUNDS[name], (dims, seed, name, gap)
            assert min(float(BC.row_cosines(a, b).min()) for a, b in zip(e32[1], e64[1])) > 0.99999
