"""The reverse mode of particle sampling on the GPU (csrc/pspec_particles.hip: cells, spread, sample_grad, coefs_adjoint; PeriodicSolver.observe,
spread, sample_gradient, particle_cells) against the float64 restatement (tests/pspec_particles_adjoint_oracle.py) on the cases of
tests/pspec_particles_adjoint_cases.py, whose bounds tests/test_oracle_pspec_particles_adjoint.py shows to tell every deliberately wrong
variant apart.  Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import pspec_particles_adjoint_cases as AC
import pspec_particles_adjoint_oracle as AO

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def setup(shape, B, name, order):
    """(solver with kappa, state of the case's fields, particles of the case's set, cotangent [B, P, 4])."""
    s = AC.solver(shape, kappa=1e-3)
    w, th = AC.fields(shape, B)
    state = s.init_vorticity(dev(w), AC.MEANS[:B])
    state.that = s.init(dev(w), dev(w), dev(th)).that
    pos = AC.positions(shape, B, name)
    return s, state, s.init_particles(dev(pos[..., 0], torch.float64), dev(pos[..., 1], torch.float64), order=order), dev(AC.cotangent(shape, B, name))


def observe_gradients(s, shape, B, name, order, fields=AC.ALL, columns=(0, 1, 2, 3), shared=False):
    """(values, wbar, thetabar, xbar, ybar) of sum(observe . r) by autograd, r the named columns of the case's cotangent."""
    w, th = (dev(a).requires_grad_(True) for a in AC.fields(shape, B))
    pos = AC.positions(shape, B, name)
    x, y = (dev(pos[0, :, k] if shared else pos[..., k], torch.float64).requires_grad_(True) for k in range(2))
    out = s.observe(w, x, y, fields=fields, theta=th, mean=AC.MEANS[:B], order=order)
    torch.sum(out * dev(AC.cotangent(shape, B, name)[..., list(columns)])).backward()
    return out.detach(), w.grad, th.grad, x.grad, y.grad


def check(what, got, ref, case):
    e = AC.rel_l2(host(got), ref)
    print('%-16s %-28s %.2e (bound %.1e)' % (what, case, e, AC.BOUND[what]))
    return e


# ---------------------------------------------------------------------------------------------------- 1. the forward
@pytest.mark.parametrize('order', AC.ORDERS)
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_the_forward_of_observe_is_bitwise_sample(gpu_device, shape, order):
    s, state, p, _ = setup(shape, 3, 'mixed', order)
    w, th = (dev(a) for a in AC.fields(shape, 3))
    for fields in (AC.ALL, ('u', 'v'), ('theta', 'u', 'u'), 'w'):
        got = s.observe(w, p.pos[..., 0].contiguous(), p.pos[..., 1].contiguous(), fields=fields, theta=th, mean=AC.MEANS, order=order)
        assert got.dtype == torch.float32 and torch.equal(got, s.sample(state, p, fields)), fields
    # positions shared by the batch
    x, y = p.pos[0, :, 0].contiguous(), p.pos[0, :, 1].contiguous()
    q = s.init_particles(x, y, order=order, batch=3)
    assert torch.equal(s.observe(w, x, y, theta=th, mean=AC.MEANS, order=order), s.sample(state, q))
    # a solver without a scalar
    s0 = AC.solver(shape)
    assert torch.equal(s0.observe(w, x, y, mean=AC.MEANS, order=order), s.sample(state, q))


# ---------------------------------------------------------------------------------------------------- 2. values against the restatement
@pytest.mark.parametrize('B', AC.BATCHES)
@pytest.mark.parametrize('order', AC.ORDERS)
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_every_result_matches_the_restatement(gpu_device, shape, order, B):
    worst = {}
    for name in AC.SETS:
        case = '%s order %d B %d %s' % (AC.shape_id(shape), order, B, name)
        ref = AC.reference(shape, B, name, order)
        s, state, p, r = setup(shape, B, name, order)
        got = dict(spread=torch.stack(s.spread(p, r)), sample_gradient=s.sample_gradient(state, p, AC.ALL))
        _, got['wbar'], got['thetabar'], got['xbar'], got['ybar'] = observe_gradients(s, shape, B, name, order)
        assert got['sample_gradient'].shape == (B, p.count, 4, 2) and got['xbar'].dtype == torch.float64
        for q in ('spread', 'sample_gradient', 'wbar', 'thetabar', 'xbar', 'ybar'):
            worst[q] = max(worst.get(q, 0.0), check(q, got[q], ref[q], case))
    for q, e in worst.items():
        assert e <= AC.BOUND[q], (q, e)


def test_one_call_at_the_longest_axis(gpu_device):
    shape, order, B, name = AC.WIDE, 6, 1, 'mixed'
    ref = AC.reference(shape, B, name, order)
    s, state, p, r = setup(shape, B, name, order)
    got = dict(spread=torch.stack(s.spread(p, r)), sample_gradient=s.sample_gradient(state, p, AC.ALL))
    _, got['wbar'], got['thetabar'], got['xbar'], got['ybar'] = observe_gradients(s, shape, B, name, order)
    # the derivative along the 1024-node axis has bounds of its own (the cases module says why)
    errs = {q: check(q + '_wide' if q in ('sample_gradient', 'xbar') else q, got[q], ref[q], '1024x64 order 6') for q in got}
    for q, e in errs.items():
        assert e <= AC.BOUND[q + '_wide' if q in ('sample_gradient', 'xbar') else q], (q, e)


def test_fields_named_in_another_order_and_shared_positions(gpu_device):
    """('theta', 'u', 'u') sums two cotangents into u's image; [P] positions shared by the grids get the sum over the grids."""
    shape, order, B = AC.OBLONG, 4, 3
    nx, ny, Lx, Ly = shape
    s = AC.solver(shape, kappa=1e-3)
    w, th = AC.fields(shape, B)
    pos, r = AC.positions(shape, B, 'mixed'), AC.cotangent(shape, B, 'mixed')[..., :3].astype(np.float64)
    fields = ('theta', 'u', 'u')
    ref = AO.observe_gradients(w, th, AC.MEANS, pos[0, :, 0], pos[0, :, 1], fields, r, Lx, Ly, order)
    got = observe_gradients(s, shape, B, 'mixed', order, fields, (0, 1, 2), shared=True)[1:]
    assert got[2].shape == (pos.shape[1],)
    for q, g, f in zip(('wbar', 'thetabar', 'xbar', 'ybar'), got, ref):
        assert check(q, g, f, 'theta,u,u shared') <= AC.BOUND[q], q


# ---------------------------------------------------------------------------------------------------- 3. the two kernels against each other
@pytest.mark.parametrize('order', AC.ORDERS)
@pytest.mark.parametrize('shape', AC.SHAPES, ids=AC.shape_id)
def test_spread_is_the_transpose_of_the_gather_kernel(gpu_device, shape, order):
    from nns import ops
    nx, ny, Lx, Ly = shape
    worst = 0.0
    for name in AC.SETS:
        s, _, p, r = setup(shape, 3, name, order)
        c = dev(np.random.default_rng(AC.SEED + order).standard_normal((4, 3, nx, ny)))
        Sc = host(ops.spec_ns_particle_sample(c, p.pos, order, Lx, Ly))
        STr = host(torch.stack(s.spread(p, r)))
        lhs, rhs = float(np.sum(Sc * host(r))), float(np.sum(host(c) * STr))
        e = abs(lhs - rhs) / (np.linalg.norm(Sc) * np.linalg.norm(host(r)))
        print('identity         %s order %d %-8s %.2e (bound %.1e)' % (AC.shape_id(shape), order, name, e, AC.BOUND['identity']))
        worst = max(worst, e)
    assert worst <= AC.BOUND['identity']


# ---------------------------------------------------------------------------------------------------- 4.-6. bits
@pytest.mark.parametrize('order', AC.ORDERS)
def test_spread_repeats_bitwise_is_independent_of_the_batch_and_leaves_exact_zeros(gpu_device, order):
    shape = AC.OBLONG
    nx, ny, Lx, Ly = shape
    for name in ('mixed', 'cluster', 'one'):
        s, _, p, r = setup(shape, 3, name, order)
        first = torch.stack(s.spread(p, r))
        for _ in range(3):
            assert torch.equal(torch.stack(s.spread(p, r)), first), name
        for b in range(3):
            alone = s.init_particles(p.pos[b:b + 1, :, 0].contiguous(), p.pos[b:b + 1, :, 1].contiguous(), order=order)
            assert torch.equal(torch.stack(s.spread(alone, r[b:b + 1].contiguous()))[:, 0], first[:, b]), (name, b)
        # nodes that no stencil covers are exactly 0, every node that one covers with a nonzero weight is not
        pos = AC.positions(shape, 3, name)
        reach = AO.spread(np.ones(pos.shape[:2]), pos[..., 0], pos[..., 1], nx, ny, Lx, Ly, order) > 0
        got = host(first)
        assert np.all(got[:, ~reach] == 0.0), name
        assert reach.sum() < reach.size and np.any(got[:, reach] != 0.0)
    # the gradients of observe repeat bitwise too
    a = observe_gradients(s, shape, 3, 'cluster', order)
    b = observe_gradients(s, shape, 3, 'cluster', order)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_particle_cells_sorts_stably_by_the_cell_of_the_gather(gpu_device):
    shape = AC.OBLONG
    nx, ny, Lx, Ly = shape
    for name in ('mixed', 'cluster', 'uniform'):
        s, _, p, _ = setup(shape, 3, name, 6)
        perm, start = s.particle_cells(p)
        assert perm.dtype == torch.int64 and start.dtype == torch.int32 and start.shape == (3 * nx * ny + 1,)
        pos = AC.positions(shape, 3, name)
        key = AO.cell_keys(pos[..., 0], pos[..., 1], nx, ny, Lx, Ly).ravel()
        ref = np.argsort(key, kind='stable')
        assert np.array_equal(perm.cpu().numpy(), ref), name
        assert np.array_equal(start.cpu().numpy(), np.searchsorted(key[ref], np.arange(3 * nx * ny + 1))), name


# ---------------------------------------------------------------------------------------------------- 7. through evolve
def chain_error():
    """|<observe'(J d), r> - <d, grad_w <observe(evolve(w)), r>>| / (|observe'(J d)| |r|): observe is linear in w, so observe' is observe on
    the tangent field, at rest."""
    shape, order, B, nsteps = AC.SQUARE, 4, 3, 2
    s = AC.solver(shape)
    w0 = AC.fields(shape, B)[0]
    d = np.random.default_rng(AC.SEED + 1).standard_normal(w0.shape).astype(np.float32)
    pos, r = AC.positions(shape, B, 'mixed'), dev(AC.cotangent(shape, B, 'mixed')[..., :3])
    x, y = dev(pos[..., 0], torch.float64), dev(pos[..., 1], torch.float64)
    fields = ('u', 'v', 'w')
    w = dev(w0).requires_grad_(True)
    out = s.observe(s.evolve(w, nsteps, mean=AC.MEANS), x, y, fields=fields, mean=AC.MEANS, order=order)
    torch.sum(out * r).backward()
    _, Jd = s.evolve_tangent(dev(w0), dev(d), nsteps, mean=AC.MEANS)
    lin = host(s.observe(Jd, x, y, fields=fields, order=order))
    lhs, rhs = float(np.sum(lin * host(r))), float(np.sum(host(w.grad) * d.astype(np.float64)))
    e = abs(lhs - rhs) / (np.linalg.norm(lin) * np.linalg.norm(host(r)))
    print('chain            64x64 order 4, 2 steps: lhs %.9e rhs %.9e  %.2e (bound %.1e)' % (lhs, rhs, e, AC.BOUND['chain']))
    return e


def test_the_chain_through_evolve_matches_the_tangent(gpu_device):
    assert chain_error() <= AC.BOUND['chain']


# ---------------------------------------------------------------------------------------------------- 8. a buoyant solver
def test_a_buoyant_solver_observes_u_and_theta(gpu_device):
    shape, order, B = AC.SQUARE, 6, 3
    nx, ny, Lx, Ly = shape
    s = AC.solver(shape, kappa=1e-3, scalar_gradient=(0.0, 1.0), buoyancy=(0.0, 1.0))
    w0, th0 = AC.fields(shape, B)
    pos, r = AC.positions(shape, B, 'mixed'), AC.cotangent(shape, B, 'mixed')[..., :2]
    fields = ('u', 'theta')
    ref = AO.observe_gradients(w0, th0, AC.MEANS, pos[..., 0], pos[..., 1], fields, r.astype(np.float64), Lx, Ly, order)
    got = observe_gradients(s, shape, B, 'mixed', order, fields, (0, 1))[1:]
    for q, g, f in zip(('wbar', 'thetabar', 'xbar', 'ybar'), got, ref):
        assert check(q, g, f, 'buoyant u,theta') <= AC.BOUND[q], q
    # and through two buoyant steps the gradient reaches both initial fields
    w, th = dev(w0).requires_grad_(True), dev(th0).requires_grad_(True)
    w1, th1 = s.evolve(w, 2, theta=th, mean=AC.MEANS)
    out = s.observe(w1, dev(pos[..., 0], torch.float64), dev(pos[..., 1], torch.float64), fields=fields, theta=th1, mean=AC.MEANS, order=order)
    torch.sum(out * dev(r)).backward()
    for g in (w.grad, th.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # theta without a scalar, and on a solver without kappa, is refused
    with pytest.raises(ValueError):
        s.observe(dev(w0), dev(pos[..., 0], torch.float64), dev(pos[..., 1], torch.float64), fields=fields)
    with pytest.raises(ValueError):
        AC.solver(shape).observe(dev(w0), dev(pos[..., 0], torch.float64), dev(pos[..., 1], torch.float64), theta=dev(th0))


# ---------------------------------------------------------------------------------------------------- 9. a nan position
@pytest.mark.parametrize('order', AC.ORDERS)
def test_a_nan_position_stays_inside_its_cell_and_its_grid(gpu_device, order):
    """Input validation with masked indices, as the forward has: no index is taken from the nan."""
    shape, B = AC.SQUARE, 3
    nx, ny, Lx, Ly = shape
    s, _, _, r = setup(shape, B, 'mixed', order)
    pos = AC.positions(shape, B, 'mixed').copy()
    pos[1, 40] = (float('nan'), 0.3 * Ly)
    pos[1, 41] = (float('inf'), float('-inf'))
    p = s.init_particles(dev(pos[..., 0], torch.float64), dev(pos[..., 1], torch.float64), order=order)
    perm, start = s.particle_cells(p)
    got = host(torch.stack(s.spread(p, r)))
    assert np.isfinite(got[:, 0]).all() and np.isfinite(got[:, 2]).all()
    # the cells the two particles were sorted into, from the table itself
    slot = {int(q): k for k, q in enumerate(perm.cpu().numpy())}
    st = start.cpu().numpy()
    allowed = np.zeros((nx, ny), dtype=bool)
    for q in (1 * pos.shape[1] + 40, 1 * pos.shape[1] + 41):
        cell = int(np.searchsorted(st, slot[q], side='right')) - 1
        assert cell // (nx * ny) == 1
        ci, cj = (cell // ny) % nx, cell % ny
        for a in range(order):
            for c in range(order):
                allowed[(ci - (order // 2 - 1) + a) % nx, (cj - (order // 2 - 1) + c) % ny] = True
    bad = ~np.isfinite(got[:, 1])
    assert bad.any() and not bad[:, ~allowed].any()
