"""The host launch layer of csrc/nns_common.h as seen through the wrappers: kernels whose dynamic-LDS size depends on their arguments are
called with a small need first and a larger one afterwards IN ONE PROCESS.  The layer remembers the largest limit it has granted per kernel
and asks the runtime only for a larger one, so the second call of each pair is the one that has to raise the limit again; a missed opt-in
is a launch error (NnsError), never a fault.  Results are held to the float64 references and tolerances of tests/test_gpu_neural.py."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _mlp(depth, width, seed):
    from nns.neural_spectral.spectral_ode import PixelMLP
    torch.manual_seed(seed)
    m = PixelMLP(depth, width).cuda()
    for b in m.biases:
        torch.nn.init.normal_(b, std=0.3)
    return [w.detach() for w in m.weights], [b.detach() for b in m.biases]


@pytest.mark.parametrize('width', [32, 64])
def test_pixel_mlp_lds_need_rises_with_depth(width, gpu_device):
    """pixel_mlp_fwd / pixel_mlp_bwd stage every layer's weights in LDS: a depth-2 stack, then a depth-8 stack of the same width class (the
    same kernel instantiation: widths <= 32, or wider), bf16 and float32 operands.  Forward: 1e-5 (float32) / 5e-2 (bf16) against the float64
    oracle; backward: 1e-2 against the oracle with bf16 operand rounding, 2e-5 (float32 operands, widths <= 32) against the unrounded one."""
    from nns import ops
    from oracle import neural as ON
    for depth in (2, 8):
        Ws, bs = _mlp(depth, width, 100 * width + depth)
        x = torch.randn(2, 3, 19, 23, device='cuda')
        gy = torch.randn(2, 3, 19, 23, device='cuda')
        args = ([w.cpu().double() for w in Ws], [b.cpu().double() for b in bs], x.cpu().double())
        ref = ON.pixel_mlp(*args).numpy()
        assert rel_l2(ops.pixel_mlp_fwd(x, Ws, bs, bf16=False).cpu().numpy(), ref) < 1e-5, (depth, width)
        assert rel_l2(ops.pixel_mlp_fwd(x, Ws, bs, bf16=True).cpu().numpy(), ref) < 5e-2, (depth, width)
        for bf16, tol in ((True, 1e-2), (False, 2e-5)):
            if not bf16 and width > 32:
                continue                                                          # the float32-operand backward serves widths <= 32
            ref_gx, ref_gW, ref_gb = ON.pixel_mlp_backward(*args, gy.cpu().double(), bf16=bf16)
            gx, gW, gb = ops.pixel_mlp_bwd(x, gy, Ws, bs, bf16=bf16)
            assert rel_l2(gx.cpu().numpy(), ref_gx.numpy()) < tol, (depth, width, bf16)
            for l in range(depth):
                assert rel_l2(gW[l].cpu().numpy(), ref_gW[l].numpy()) < tol, (depth, width, bf16, l)
                assert rel_l2(gb[l].cpu().numpy(), ref_gb[l].numpy()) < tol, (depth, width, bf16, l)


@pytest.mark.parametrize('K', [30, 48])
def test_adjoint_chain_lds_need_rises_with_nt(K, gpu_device):
    """ode_adjoint_chain keeps min(Nt, what fits) step Jacobians per LDS buffer: Nt = 2 (two steps' worth), then Nt = 60 (full buffers, several
    chunks), for the 32-row (K <= 32) and the 64-row instantiation.  1e-5 against the float64 recurrence of test_adjoint_chain_kernel_paths."""
    from nns import ops
    for Nt in (2, 60):
        g0 = torch.Generator().manual_seed(100 * Nt + K)
        J = (torch.randn(Nt, 2, K, K, generator=g0) * (0.5 / K ** 0.5) + torch.eye(K)).float()
        g = torch.randn(Nt, 2, K, generator=g0).float()
        lam = ops.ode_adjoint_chain(J.cuda(), g.cuda()).cpu().double()
        ref = torch.empty(Nt, 2, K, dtype=torch.float64)
        ref[Nt - 1] = g[Nt - 1].double()
        for s in range(Nt - 1, 0, -1):
            ref[s - 1] = g[s - 1].double() + torch.einsum('bi,bij->bj', ref[s], J[s].double())
        assert rel_l2(lam.numpy(), ref.numpy()) < 1e-5, (Nt, K)


def test_halfsweep_rejects_half_precision_before_any_launch(gpu_device):
    """A float16 slab used to reach the float64 half-sweep kernel; it is a TypeError now, raised before the library is called."""
    from nns import _lib, ops
    p = torch.zeros(8, 8, dtype=torch.float16, device='cuda')
    C = torch.zeros_like(p)
    err = torch.zeros(1, dtype=torch.float16, device='cuda')
    rec = _lib.CallRecorder()
    with rec.stage('half'):
        with pytest.raises(TypeError):
            ops.fd_sor_redblack_halfsweep_(p, C, err, 0, 0, 0.1, 0.1, 1.5)
        with pytest.raises(TypeError):
            ops.fd_sor_redblack_halfsweep_gated_(p, C, err, err.clone(), 1e-6, 0, 0, 0.1, 0.1, 1.5)
    assert rec.stages['half'] == []
    assert not bool(p.any()) and not bool(err.any())
