"""The fused ODEFunc integrator (csrc/ode_mlp_kernels.hip) pinned on each of its paths, at the cases, the bound and the exact read-outs of
tests/ode_cases.py (its docstring has the dispatch rules, the reasoning behind the bound and the figures measured on an MI355X):

  * row forward (ops.ode_mlp_fwd) and tile forward (the same call in ONE child process with NNS_ODE_ROW_MAX=0) against the oracle trajectory;
  * sequential backward (ops.ode_mlp_bwd on the row-forward states) and independent single steps (ops.ode_mlp_bwd_steps, free dt) against
    the oracle's gradients;
  * the time-parallel composition and the dispatch between the two through odesolver(...).backward() with anode._parallel_rows set, the
    branch taken asserted by counting the ops calls;
  * bitwise repeatability where the kernel promises it;
  * elu1 and its derivative read out bit for bit on 2048 values of z.

Every path is called directly or forced, so the card's CU count never chooses the kernel under test.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ode_cases as OC
from ode_cases import rel_l2

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize('K,mb,Nt,method', OC.CASE_METHODS, ids=OC.CASE_METHOD_IDS)


def dev(K, mb, Nt):
    mlp, z0, w = OC.inputs(K, mb, Nt)
    return [p.cuda() for p in mlp], z0.cuda(), w.cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def check(tag, got, ref, names, bound):
    """Prints every figure, then asserts them all."""
    errs = {q: rel_l2(got[q].detach().cpu().numpy(), ref[q]) for q in names}
    print('ode_mlp %s: bound %.2e  %s' % (tag, bound, '  '.join('%s %.2e' % (q, errs[q]) for q in names)))
    assert all(np.isfinite(got[q].detach().cpu().numpy()).all() for q in names), tag
    assert max(errs.values()) <= bound, (tag, bound, errs)


def sequential(K, mb, Nt, method):
    from nns import ops
    mlp, z0, w = dev(K, mb, Nt)
    states = ops.ode_mlp_fwd(z0, *mlp, Nt, method)
    gz0, gs = ops.ode_mlp_bwd(z0, *mlp, states, w, Nt, method)
    return dict(zip(OC.QUANTITIES, [states, gz0] + list(gs)))


# ------------------------------------------------------------------------------------------------------------------ forward
@CASES
def test_row_forward(K, mb, Nt, method, gpu_device):
    from nns import ops
    assert os.environ.get('NNS_ODE_ROW_MAX') is None                # the default: the row kernel up to mb = 4096
    mlp, z0, _ = dev(K, mb, Nt)
    out = ops.ode_mlp_fwd(z0, *mlp, Nt, method)
    assert out.shape == (Nt, mb, K)
    check('row forward ' + OC.case_id(K, mb, Nt, method), {'traj': out}, OC.oracle(K, mb, Nt, method), ('traj',), OC.bound(K, mb, Nt, method))


@pytest.fixture(scope='module')
def tile_child(tmp_path_factory, gpu_device):
    """Every case and scheme and the elu1 read-out through the 16-row MFMA tile kernel: ONE child process (NNS_ODE_ROW_MAX is read once per
    process), one .npz."""
    from conftest import PKG, ROOT
    path = str(tmp_path_factory.mktemp('ode_tile') / 'tile.npz')
    code = ("import sys\n"
            "sys.path[:0] = [%r, %r, %r]\n"
            "import ode_cases\n"
            "ode_cases.tile_child(sys.argv[1])\n" % (os.path.join(ROOT, 'tests'), ROOT, PKG))
    r = subprocess.run([sys.executable, '-c', code, path], env=dict(os.environ, NNS_ODE_ROW_MAX='0'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@CASES
def test_tile_forward(K, mb, Nt, method, tile_child, gpu_device):
    out = tile_child[OC.case_id(K, mb, Nt, method)]
    assert out.shape == (Nt, mb, K)
    check('tile forward ' + OC.case_id(K, mb, Nt, method), {'traj': torch.from_numpy(out)}, OC.oracle(K, mb, Nt, method), ('traj',),
          OC.bound(K, mb, Nt, method))


def test_tile_child_ran_another_kernel(tile_child, gpu_device):
    """The two forward kernels sum in different orders: were the child's results bitwise the row kernel's on all 30 trajectories, it ran the row kernel."""
    from nns import ops
    differ = 0
    for K, mb, Nt, method in OC.CASE_METHODS:
        mlp, z0, _ = dev(K, mb, Nt)
        row = ops.ode_mlp_fwd(z0, *mlp, Nt, method).cpu()
        differ += not torch.equal(bits(row), bits(torch.from_numpy(tile_child[OC.case_id(K, mb, Nt, method)])))
    assert differ >= 15, differ


# ------------------------------------------------------------------------------------------------------------------ backward
@CASES
def test_sequential_backward(K, mb, Nt, method, gpu_device):
    """ops.ode_mlp_bwd, one launch over all Nt steps, on the row-forward states: gz0 and the six parameter gradients."""
    got = sequential(K, mb, Nt, method)
    check('sequential backward ' + OC.case_id(K, mb, Nt, method), got, OC.oracle(K, mb, Nt, method), OC.GRADS, OC.bound(K, mb, Nt, method))


@pytest.mark.parametrize('K,rows,method', OC.STEP_CASES, ids=OC.STEP_IDS)
def test_independent_steps_backward(K, rows, method, gpu_device):
    """ops.ode_mlp_bwd_steps with a dt that is no 1 / Nt against the oracle's single step; grad_y without the parameter gradients (NULL
    pointers: the kernel skips their products and atomics) is bitwise grad_y with them."""
    from nns import ops
    mlp, y, g = OC.step_inputs(K, rows)
    mlp, y, g = [p.cuda() for p in mlp], y.cuda(), g.cuda()
    gy, gs = ops.ode_mlp_bwd_steps(y, *mlp, g, OC.STEP_DT, method)
    gy_only, none = ops.ode_mlp_bwd_steps(y, *mlp, g, OC.STEP_DT, method, want_param_grads=False)
    assert none is None
    assert torch.equal(bits(gy_only), bits(gy))
    check('independent steps K%d rows%d %s' % (K, rows, method), dict(zip(OC.STEP_GRADS, [gy] + list(gs))), OC.step_oracle(K, rows, method),
          OC.STEP_GRADS, OC.step_bound(K, rows, method))


class _Counted:
    def __init__(self, monkeypatch):
        from nns import ops
        self.n = {}
        for name in ('ode_mlp_fwd', 'ode_mlp_bwd', 'ode_mlp_bwd_steps', 'ode_adjoint_chain'):
            self.n[name] = 0
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def counted(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return counted


def through_autograd(K, mb, Nt, method, parallel_rows, monkeypatch):
    """odesolver(ODEFunc, z0).backward() with the time-parallel limit set: the quantities, and how often each op was called."""
    from nns.neural_spectral import anode
    from nns.neural_spectral.spectral_ode import ODEFunc
    mlp, z0, w = dev(K, mb, Nt)
    f = ODEFunc(K).cuda()
    params = [f.net[0].weight, f.net[0].bias, f.net[2].weight, f.net[2].bias, f.net[4].weight, f.net[4].bias]
    with torch.no_grad():
        for p, v in zip(params, mlp):
            p.copy_(v)
    z0.requires_grad_(True)
    monkeypatch.setattr(anode, '_parallel_rows', parallel_rows)
    calls = _Counted(monkeypatch)
    out = anode.odesolver(f, z0, {'Nt': Nt, 'method': method})
    (out * w).sum().backward()
    monkeypatch.undo()
    return dict(zip(OC.QUANTITIES, [out.detach(), z0.grad] + [p.grad for p in params])), calls.n


@CASES
def test_time_parallel_backward(K, mb, Nt, method, monkeypatch, gpu_device):
    """anode._parallel_rows = 10**9: every case with Nt > 1 goes through Jacobians (steps without parameter gradients), chain, steps -- held to
    the oracle bound; Nt == 1 has nothing to parallelise and takes the one sequential launch."""
    got, n = through_autograd(K, mb, Nt, method, 10 ** 9, monkeypatch)
    if Nt > 1:
        assert n == {'ode_mlp_fwd': 1, 'ode_mlp_bwd': 0, 'ode_mlp_bwd_steps': 2, 'ode_adjoint_chain': 1}, n
    else:
        assert n == {'ode_mlp_fwd': 1, 'ode_mlp_bwd': 1, 'ode_mlp_bwd_steps': 0, 'ode_adjoint_chain': 0}, n
    check('time-parallel backward ' + OC.case_id(K, mb, Nt, method), got, OC.oracle(K, mb, Nt, method), OC.QUANTITIES, OC.bound(K, mb, Nt, method))


@CASES
def test_dispatch_sequential_is_the_direct_call(K, mb, Nt, method, monkeypatch, gpu_device):
    """anode._parallel_rows = 0: one ops.ode_mlp_bwd call, and bitwise its result.  Up to two row tiles (mb <= 32) that includes the parameter
    gradients: an address receives one atomic per workgroup on a zeroed buffer, and a + b = b + a.  From three tiles on the order of the
    atomics is free; two orders of a sum of n <= 4 float32 terms are each within (n - 1) 2^-24 sum|a_i| of the exact sum, so they differ by
    at most 6 x 2^-24 = 3.6e-7 of sum|a_i|: held to 1e-6 rel-L2 there (bitwise in practice), and gz0, which no atomic touches, bitwise."""
    got, n = through_autograd(K, mb, Nt, method, 0, monkeypatch)
    assert n == {'ode_mlp_fwd': 1, 'ode_mlp_bwd': 1, 'ode_mlp_bwd_steps': 0, 'ode_adjoint_chain': 0}, n
    want = sequential(K, mb, Nt, method)
    for q in ('traj', 'gz0'):
        assert torch.equal(bits(got[q]), bits(want[q])), q
    for q in OC.GRADS[1:]:
        if mb <= 2 * OC.TB:
            assert torch.equal(bits(got[q]), bits(want[q])), q
        else:
            assert rel_l2(got[q].cpu().numpy(), want[q].cpu().numpy()) <= 1e-6, q


@pytest.mark.parametrize('K,mb,Nt', OC.SHAPES, ids=[OC.case_id(*s) for s in OC.SHAPES])
def test_repeatable(K, mb, Nt, gpu_device):
    """gz0 is bitwise repeatable on every case (no atomic touches it); the parameter gradients too while an address receives at most two
    atomics (mb <= 32; one workgroup, mb <= 16, issues one per address)."""
    for method in OC.METHODS:
        a, b = sequential(K, mb, Nt, method), sequential(K, mb, Nt, method)
        for q in OC.QUANTITIES:
            if q in ('traj', 'gz0') or mb <= 2 * OC.TB:
                assert torch.equal(bits(a[q]), bits(b[q])), (method, q)


@pytest.mark.parametrize('K,mb,Nt', [(17, 33, 5), (1, 17, 2), (31, 17, 3), (16, 1, 1)], ids=lambda v: str(v))
def test_output_guards_untouched(K, mb, Nt, gpu_device):
    """nns_ode_mlp_fwd_f32 and nns_ode_mlp_bwd_f32 called directly with the trajectory, gz0, the six parameter gradients and the workspace
    inside ONE buffer of sentinels, ragged tiles and padded columns: nothing between them is written (the `row0 + b < mb`, `k < K` and
    `nn < K` conditions on the stores and atomics, the workspace size), and what is written is what the ops wrappers return."""
    from nns import _lib
    L = _lib.lib()
    H, guard, sentinel = OC.H, 1024, -12345.5
    mlp, z0, w = dev(K, mb, Nt)
    sizes = [('traj', Nt * mb * K), ('gz0', mb * K), ('gW0', H * K), ('gb0', H), ('gW1', H * H), ('gb1', H), ('gW2', K * H), ('gb2', K),
             ('work', L.nns_ode_mlp_bwd_workspace(mb) // 4)]
    buf = torch.full((guard + sum(n + guard for _, n in sizes),), sentinel, device='cuda')
    off, o = {}, guard
    for name, n in sizes:
        off[name] = (o, n)
        o += n + guard
    ptr = lambda name: buf.data_ptr() + 4 * off[name][0]
    stream = torch.cuda.current_stream().cuda_stream
    for method in OC.METHODS:
        buf.fill_(sentinel)
        ins = [z0.data_ptr()] + [p.data_ptr() for p in mlp]
        rc = L.nns_ode_mlp_fwd_f32(*ins, ptr('traj'), mb, K, H, Nt, OC.METHODS.index(method), stream)
        assert rc == 0, L.nns_last_error()
        rc = L.nns_ode_mlp_bwd_f32(*ins, ptr('traj'), w.data_ptr(), *[ptr(q) for q in OC.GRADS], ptr('work'), mb, K, H, Nt, OC.METHODS.index(method), stream)
        assert rc == 0, L.nns_last_error()
        torch.cuda.synchronize()
        host = buf.cpu()
        keep = torch.ones(len(host), dtype=torch.bool)
        for name, (o, n) in off.items():
            keep[o:o + n] = False
        assert int(keep.sum()) == guard * (len(sizes) + 1) and bool((host[keep] == sentinel).all()), (method, (host[keep] != sentinel).nonzero()[:8].tolist())
        want = sequential(K, mb, Nt, method)
        for q in OC.QUANTITIES:
            o, n = off[q]
            assert not bool((host[o:o + n] == sentinel).any()), (method, q)                 # and every element of every result is written
            if q in ('traj', 'gz0') or mb <= 2 * OC.TB:
                assert torch.equal(bits(host[o:o + n]), bits(want[q].cpu().reshape(-1))), (method, q)


# ------------------------------------------------------------------------------------------------------------------ elu1, exactly
def _elu_report(tag, z, got):
    rel, neg = OC.elu_errors(z, got)
    zs = np.asarray(z, dtype=np.float32).ravel()[neg]
    i = int(np.argmax(rel))
    below = zs <= np.float32(OC.ELU_SPLIT)
    print('elu1 %s: worst relative error %.3e at z = %.9g;  exp2 branch %.3e at z = %.9g;  polynomial branch %.3e at z = %.9g' % (
        tag, rel[i], zs[i], rel[below].max(), zs[below][np.argmax(rel[below])], rel[~below].max(), zs[~below][np.argmax(rel[~below])]))
    assert rel.max() <= OC.ELU_REL, (tag, rel[i], zs[i])


def test_elu1_row_kernel(gpu_device):
    """out[j] is bit for bit the row kernel's elu1(b1[32 q + j]) (ode_cases.elu_setup): z > 0 bitwise, exactly -1 in the underflow region,
    <= 1e-6 relative to float64 expm1 -- twice the 5e-7 claimed in the kernel's comment, which is the thing under test.
    Measured: see the docstring of tests/ode_cases.py."""
    from nns import ops
    z = OC.elu_points()
    _elu_report('row kernel', z.numpy(), OC.elu_readout(ops, z).numpy())


def test_elu1_tile_kernel(tile_child, gpu_device):
    _elu_report('tile kernel', OC.elu_points().numpy(), tile_child['elu'])


def test_elu_derivative_and_relu_tie(gpu_device):
    """The same setup through ops.ode_mlp_bwd with grad_out = 1: gb1[32 q + j] is the kernel's elu' (h + 1 below 0) -- within 6e-7 absolute
    of exp(min(z, 0)): |h| <= 1 times the 5e-7 claim plus one float32 rounding of h + 1 -- and every unselected gb1 exactly 0.  z1 = 0
    everywhere puts every ReLU on its tie: gb0 and gW0 exactly 0 and gz0 bitwise grad_out, torch's relu'(0) = 0."""
    from nns import ops
    worst, worst_z = 0.0, 0.0
    ones = torch.ones(1, 1, OC.ELU_K, device='cuda')
    for b1 in OC.elu_points():
        for q in range(OC.H // 32):
            args = OC.elu_setup(b1, q, 'cuda')
            states = ops.ode_mlp_fwd(*args, 1, 'Euler')
            gz0, (gW0, gb0, gW1, gb1, gW2, gb2) = ops.ode_mlp_bwd(*args, states, ones, 1, 'Euler')
            sel = torch.zeros(OC.H, dtype=torch.bool)
            sel[32 * q:32 * q + 32] = True
            gb1 = gb1.cpu()
            assert bool((gb1[~sel] == 0).all()), q
            z = b1[sel].double()
            err = (gb1[sel].double() - torch.exp(torch.clamp(z, max=0))).abs()
            if float(err.max()) > worst:
                worst, worst_z = float(err.max()), float(z[int(err.argmax())])
            assert bool((gb1[sel][z > 0] == 1).all())
            assert bool((gb0 == 0).all()) and bool((gW0 == 0).all()) and bool((gW1 == 0).all())            # h1 = relu(0) = 0, relu'(0) = 0
            assert torch.equal(bits(gz0), bits(ones[0]))
            assert torch.equal(bits(gb2), bits(ones[0, 0]))
    print("elu' worst absolute error %.3e at z = %.9g" % (worst, worst_z))
    assert worst <= OC.ELU_GRAD_ABS, (worst, worst_z)
