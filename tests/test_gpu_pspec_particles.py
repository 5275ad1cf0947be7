"""The Lagrangian tracers of PeriodicSolver on the GPU (csrc/pspec_particles.hip) against the float64 restatement
(tests/pspec_particles_oracle.py) on the cases of tests/pspec_particles_cases.py, whose bounds tests/test_oracle_pspec_particles.py shows to
tell every deliberately wrong variant apart.  Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import pspec_oracle as O
import pspec_particles_cases as PC
import pspec_particles_oracle as PO

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def setup(kind, shape, order=4, stochastic=False, npart=PC.P):
    """(solver, state, particles) of a kind at a shape, the particles at positions(shape)."""
    d = PC.inputs(shape)
    s = PC.solver(kind, shape, stochastic)
    state = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']) if kind == 'buoyant' else None)
    pos = PC.positions(shape, npart)
    return s, state, s.init_particles(pos[..., 0], pos[..., 1], order=order, device='cuda')


# ---------------------------------------------------------------------------------------------------- 1. coefficients and samples
@pytest.mark.parametrize('order', PC.ORDERS)
@pytest.mark.parametrize('shape', PC.SHAPES, ids=PC.shape_id)
def test_coefficients_and_samples_match_the_restatement(gpu_device, shape, order):
    s, state, p = setup('buoyant', shape, order)
    coef_ref, val_ref = PC.oracle_read(shape, order)
    coef = s.particle_coefficients(state, PC.FIELDS, order)
    vals = s.sample(state, p, PC.FIELDS)
    assert vals.shape == (PC.B, PC.P, 4) and vals.dtype == torch.float32
    for k, f in enumerate(PC.FIELDS):
        ec, es = PC.rel_max(host(coef[k]), coef_ref[f]), PC.rel_max(host(vals[..., k]), val_ref[f])
        print('%s order %d %-5s coef %.2e sample %.2e' % (PC.shape_id(shape), order, f, ec, es))
        assert ec <= PC.COEF_BOUND and es <= PC.SAMPLE_BOUND, (f, ec, es)
    # the order of the names is the caller's, and a name may repeat
    again = s.sample(state, p, ('theta', 'u', 'u'))
    assert torch.equal(again[..., 0], vals[..., 3]) and torch.equal(again[..., 1], vals[..., 0]) and torch.equal(again[..., 2], vals[..., 0])
    assert torch.equal(s.sample(state, p)[..., 1], vals[..., 1])


def test_one_call_at_the_longest_axis(gpu_device):
    shape = PC.WIDE
    nx, ny, Lx, Ly = shape
    d = PC.inputs(shape)
    s = PC.solver('plain', shape)
    state = s.init(dev(d['u0']), dev(d['v0']))
    pos = PC.positions(shape)
    p = s.init_particles(pos[..., 0], pos[..., 1], order=4, device='cuda')
    S, w, mean, _ = PC.start('plain', shape)
    ref = PO.Tracers(S, 4).sample(w, mean, pos)
    got = host(s.sample(state, p))
    for k, f in enumerate(('u', 'v')):
        e = PC.rel_max(got[..., k], ref[..., k])
        print('1024x64 %s sample %.2e' % (f, e))
        assert e <= PC.SAMPLE_BOUND


# ---------------------------------------------------------------------------------------------------- 2. analytic flows
def test_a_base_at_rest_with_a_mean_flow(gpu_device):
    nx, ny, Lx, Ly = shape = PC.OBLONG
    U = np.array(PC.MEANS, dtype=np.float32)
    s = PC.solver('plain', shape)
    z = torch.zeros((PC.B, nx, ny), dtype=torch.float32, device='cuda')
    state = s.init(z + dev(U[:, 0])[:, None, None], z + dev(U[:, 1])[:, None, None])
    pos0 = PC.positions(shape)
    for order in PC.ORDERS:
        p = s.init_particles(pos0[..., 0], pos0[..., 1], order=order, device='cuda')
        got = host(s.sample(state, p))
        for b in range(PC.B):
            for k in range(2):
                if U[b, k] != 0:
                    e = np.abs(got[b, :, k] - float(U[b, k])).max() / abs(float(U[b, k]))
                    print('rest order %d grid %d component %d: %.2e' % (order, b, k, e))
                    assert e <= 1e-6
                else:
                    assert np.abs(got[b, :, k]).max() == 0.0
        st = state.clone()
        s.advect(st, p, 8)
        move = 8 * s.dt * U.astype(np.float64)[:, None, :]
        e = np.abs(host(p.pos) - (pos0 + move)).max() / np.abs(move).max()
        print('rest order %d trajectory: %.2e of the displacement' % (order, e))
        assert e <= 1e-6


def test_a_steady_shear_carries_particles_along_straight_lines(gpu_device):
    """u = U0 + A sin(k y), v = 0, nu = 0: x(t) = x0 + (U0 + A sin(k y0)) t.  The kernel is held to the analytic line within the restatement's
    own distance from it (the spline's error, float64) plus the advect bound."""
    from nns.periodic import PeriodicSolver
    nx, ny, Lx, Ly = shape = PC.OBLONG
    U0, A, m, nsteps = 0.4, 0.8, 2, 8
    dt = PC.inputs(shape)['dt']
    y = Ly * np.arange(ny) / ny
    u0 = np.broadcast_to(U0 + A * np.sin(2 * np.pi * m * y / Ly), (PC.B, nx, ny)).astype(np.float32)
    s = PeriodicSolver(nx, ny, dt, PC.RHO, 0.0, Lx, Ly)
    state = s.init(dev(u0), torch.zeros((PC.B, nx, ny), dtype=torch.float32, device='cuda'))
    pos0 = PC.positions(shape)
    line = pos0.copy()
    line[..., 0] += nsteps * dt * (U0 + A * np.sin(2 * np.pi * m * pos0[..., 1] / Ly))
    S = O.Scheme(nx, ny, dt, PC.RHO, 0.0, Lx, Ly)
    w, mean = S.init(u0, np.zeros_like(u0))
    for order in PC.ORDERS:
        ref = PO.Tracers(S, order).advect(w, mean, pos0, nsteps)[2]
        own = PC.displacement_error(ref, line, pos0)
        p = s.init_particles(pos0[..., 0], pos0[..., 1], order=order, device='cuda')
        s.advect(state.clone(), p, nsteps)
        e = PC.displacement_error(host(p.pos), line, pos0)
        print('shear order %d: gpu %.2e, restatement %.2e of the displacement from the line' % (order, e, own))
        assert e <= own + PC.ADVECT_BOUND


# ---------------------------------------------------------------------------------------------------- 3. advect against the restatement
@pytest.mark.parametrize('scheme,nsteps', PC.SCHEMES)
@pytest.mark.parametrize('kind', PC.KINDS)
def test_advect_matches_the_restatement(gpu_device, kind, scheme, nsteps):
    shape = PC.SQUARE
    pos0 = PC.positions(shape)
    for order in PC.ORDERS if kind == 'plain' else (4,):
        s, state, p = setup(kind, shape, order)
        twin = state.clone()
        out = s.advect(state, p, nsteps, scheme)
        assert out[0] is state and out[1] is p and state.steps == nsteps
        e = PC.displacement_error(host(p.pos), PC.oracle_advect(kind, shape, scheme, nsteps, order), pos0)
        print('%s %s %d steps order %d: %.2e of the displacement' % (kind, scheme, nsteps, order, e))
        assert e <= PC.ADVECT_BOUND
        s.step(twin, nsteps)                                              # the flow is step's, bitwise
        assert torch.equal(state.what, twin.what) and (state.that is None or torch.equal(state.that, twin.that))


def test_advect_on_the_oblong_box(gpu_device):
    shape = PC.OBLONG
    s, state, p = setup('plain', shape, 6)
    s.advect(state, p, 4)
    e = PC.displacement_error(host(p.pos), PC.oracle_advect('plain', shape, 'rk4', 4, 6), PC.positions(shape))
    print('oblong rk4 4 steps order 6: %.2e of the displacement' % e)
    assert e <= PC.ADVECT_BOUND


# ---------------------------------------------------------------------------------------------------- 4. bitwise properties
@pytest.mark.parametrize('scheme', ('rk4', 'heun'))
def test_the_state_is_bitwise_steps_on_a_stochastic_solver(gpu_device, scheme):
    s, state, p = setup('forced', PC.SQUARE, stochastic=True)
    twin = state.clone()
    s.advect(state, p, 4, scheme)
    s.step(twin, 4)
    assert torch.equal(state.what, twin.what)
    assert int(state.clock.item()) == 4 and int(twin.clock.item()) == 4 and state.steps == 4
    assert not torch.equal(state.what, PC.solver('forced', PC.SQUARE).step(s.init(*(dev(PC.inputs(PC.SQUARE)[k]) for k in ('u0', 'v0'))), 4).what)


@pytest.mark.parametrize('scheme', ('rk4', 'heun'))
def test_one_call_is_bitwise_many_and_two_runs_are_equal(gpu_device, scheme):
    s, state, p = setup('linear', PC.SQUARE, 6)
    s2, p2 = state.clone(), p.clone()
    s3, p3 = state.clone(), p.clone()
    s.advect(state, p, 8, scheme)
    for _ in range(4):
        s.advect(s2, p2, 2, scheme)
    s.advect(s3, p3, 8, scheme)
    assert torch.equal(p.pos, p2.pos) and torch.equal(state.what, s2.what) and s2.steps == 8
    assert torch.equal(p.pos, p3.pos) and torch.equal(state.what, s3.what)
    assert not torch.equal(p.pos, dev(PC.positions(PC.SQUARE), torch.float64))


def test_a_subset_of_particles_and_a_single_grid_give_the_same_bits(gpu_device):
    shape = PC.SQUARE
    s, state, p = setup('plain', shape)
    vals = s.sample(state, p, ('u', 'v', 'w'))
    sub = s.init_particles(p.pos[:, ::3, 0], p.pos[:, ::3, 1], order=4)
    assert sub.count == (PC.P + 2) // 3
    assert torch.equal(s.sample(state, sub, ('u', 'v', 'w')), vals[:, ::3])
    d = PC.inputs(shape)
    b = 1
    alone = s.init(dev(d['u0'][b:b + 1]), dev(d['v0'][b:b + 1]))
    assert torch.equal(alone.what[0], state.what[b])
    pa = s.init_particles(p.pos[b, :, 0], p.pos[b, :, 1], order=4)
    assert pa.batch == 1 and torch.equal(s.sample(alone, pa, ('u', 'v', 'w'))[0], vals[b])
    one = s.init_particles(p.pos[:, 7:8, 0], p.pos[:, 7:8, 1], order=4)      # P = 1
    assert torch.equal(s.sample(state, one, ('u', 'v', 'w')), vals[:, 7:8])
    st, sa, s1 = state.clone(), alone.clone(), state.clone()
    s.advect(state, p, 4)
    s.advect(st, sub, 4)
    s.advect(sa, pa, 4)
    s.advect(s1, one, 4)
    assert torch.equal(sub.pos, p.pos[:, ::3]) and torch.equal(pa.pos[0], p.pos[b]) and torch.equal(one.pos, p.pos[:, 7:8])
    assert torch.equal(sa.what[0], state.what[b])


@pytest.mark.parametrize('scheme,nsteps', (('rk4', 2), ('heun', 3)))
def test_eager_equals_graph_replay(gpu_device, scheme, nsteps):
    s, eager, pe = setup('forced', PC.SQUARE, stochastic=True)
    s.advect(eager.clone(), pe.clone(), nsteps, scheme)                   # loads the code objects
    st, p = eager.clone(), pe.clone()
    s.advect(eager, pe, nsteps, scheme)
    s.advect(eager, pe, nsteps, scheme)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.advect(st, p, nsteps, scheme)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(p.pos, pe.pos) and torch.equal(st.what, eager.what)
    assert int(st.clock.item()) == 2 * nsteps


# ---------------------------------------------------------------------------------------------------- 5. the Python-level refusals
def test_value_errors(gpu_device):
    s, state, p = setup('plain', PC.SQUARE)
    with pytest.raises(ValueError, match='even'):
        s.advect(state, p, 3)
    with pytest.raises(ValueError, match='scheme'):
        s.advect(state, p, 2, scheme='euler')
    with pytest.raises(ValueError, match='nsteps'):
        s.advect(state, p, -2)
    with pytest.raises(ValueError, match='theta'):
        s.sample(state, p, ('u', 'theta'))
    with pytest.raises(ValueError, match='not one of'):
        s.sample(state, p, ('u', 'p'))
    with pytest.raises(ValueError, match='at least one'):
        s.sample(state, p, ())
    with pytest.raises(ValueError, match='order'):
        s.init_particles([0.0], [0.0], order=5)
    with pytest.raises(ValueError, match='order'):
        s.particle_coefficients(state, order=3)
    with pytest.raises(ValueError, match='share the shape'):
        s.init_particles(np.zeros(3), np.zeros(4))
    two = s.init_particles(np.zeros((2, 5)), np.zeros((2, 5)), device='cuda')
    with pytest.raises(ValueError, match='grids'):
        s.advect(state, two, 2)
    with pytest.raises(ValueError, match='grids'):
        s.sample(state, two)
    other = PC.solver('plain', PC.OBLONG)
    with pytest.raises(ValueError, match='another solver'):
        other.sample(other.init(*(dev(PC.inputs(PC.OBLONG)[k]) for k in ('u0', 'v0'))), p)
    with pytest.raises(TypeError):
        s.advect(state, p.pos, 2)
    assert state.steps == 0 and torch.equal(p.pos, dev(PC.positions(PC.SQUARE), torch.float64))
    shared = s.init_particles(np.linspace(0, 1, 5, dtype=np.float32), torch.linspace(0, 1, 5), batch=PC.B, device='cuda')
    assert shared.pos.shape == (PC.B, 5, 2) and shared.pos.dtype == torch.float64 and shared.pos.is_cuda
    w = p.wrapped()
    assert float(w.min()) >= 0.0 and float(w[..., 0].max()) <= s.Lx and float(w[..., 1].max()) <= s.Ly
    assert torch.equal(s.advect(state, p, 0)[1].pos, p.pos)
