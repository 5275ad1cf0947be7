"""Measures the reverse mode of the periodic spectral solver (nns.periodic.PeriodicSolver.advance: nns_spec_ns_step_adjoint_f32 of
csrc/pspec_kernels.hip).  Writes ONE JSON record to OUTDIR/pspec_adjoint_run.json and prints it.

    python tools/pspec_adjoint_run.py OUTDIR [--steps 20] [--reps 7] [--commit ID] [--parent-lib PATH] [--no-accuracy] [--no-torch]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow, Kolmogorov force k = 4, drag 0.1) these take turns within every repetition, each from the
same saved state: the forward step (one call of `steps` steps), the forward of ``advance`` (one-step calls with a device copy of the start
spectrum between them), the adjoint call alone, forward + backward through ``advance`` (autograd, a differentiable forcing) and, unless
--no-torch, forward + backward of the same scheme composed from torch.fft ops in float32 under torch autograd.  With --parent-lib also the
forced and the unforced step of another build of the library (the parent commit's) loaded into the same process, and whether they give the
same bits.  A timing is device events around the work, reported per step as the median over the repetitions with the spread
(max - min) / median; ratios are medians of the per-repetition ratios.  The model to compare against: 7/8 of a forward step for the
recomputation plus four adjoint stages of about a scalar-step stage (1.7x a flow stage) each, 2.6x a forward step.
Accuracy (tests/pspec_adjoint_cases.py, the figures tests/test_gpu_pspec_adjoint.py bounds): wbar and gbar after 3 steps against the float64
restatement.  The register and scratch figures of the new kernels come from the code object's metadata (--isa-notes FILE: the text of
`llvm-readelf --notes` on the library, made at build time)."""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pspec_oracle as O  # noqa: E402
from nns import ops  # noqa: E402
from nns.periodic import PeriodicSolver, PeriodicState  # noqa: E402

CASES = [(256, 64), (1024, 8)]
DT, NU, DRAG = 1e-3, 1e-3, 0.1


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts, per):
    med = float(np.median(ts))
    return dict(ms=round(med / per, 5), spread=round((max(ts) - min(ts)) / med, 4))


def ratio(a, b):
    r = np.array(a) / np.array(b)
    return dict(median=round(float(np.median(r)), 4), min=round(float(r.min()), 4), max=round(float(r.max()), 4))


def dev(a):
    return torch.as_tensor(np.array(a), dtype=torch.float32, device='cuda')


def parent_steps(path):
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_forced_f32.argtypes = [P] * 3 + [I, P, Z] + [I] * 3 + [D] * 5 + [I, P]
    L.nns_spec_ns_step_f32.argtypes = [P] * 3 + [Z] + [I] * 3 + [D] * 4 + [I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def check(rc):
        if rc != 0:
            raise RuntimeError('the parent library refused the step: %d' % rc)

    def forced(s, st, n):
        check(L.nns_spec_ns_step_forced_f32(st.what.data_ptr(), st.mean.data_ptr(), s.ghat.data_ptr(), int(s.ghat.shape[0]), st.work.data_ptr(),
                                            st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, n, stream()))

    def unforced(s, st, n):
        check(L.nns_spec_ns_step_f32(st.what.data_ptr(), st.mean.data_ptr(), st.work.data_ptr(), st.work.numel(), st.batch, s.nx, s.ny, s.Lx,
                                     s.Ly, s.dt, s.nu, n, stream()))
    return dict(forced=forced, unforced=unforced)


class TorchScheme(object):
    """The same Lawson RK4 scheme from torch.fft ops in float32, for torch autograd (the comparison, not the product)."""

    def __init__(self, n, dt, nu, drag):
        m = torch.fft.fftfreq(n, 1.0 / n, device='cuda')
        j = torch.arange(n // 2 + 1, device='cuda', dtype=torch.float32)
        self.kx, self.ky = m[:, None], j[None, :]
        k2 = self.kx ** 2 + self.ky ** 2
        self.M = ((3 * m.abs()[:, None] < n) & (3 * j[None, :] < n) & (k2 > 0)).float()
        self.ik2 = torch.where(k2 > 0, 1.0 / torch.where(k2 > 0, k2, torch.ones_like(k2)), torch.zeros_like(k2))
        self.E, self.E2 = torch.exp(-(nu * k2 + drag) * dt / 2), torch.exp(-(nu * k2 + drag) * dt)
        self.n, self.dt = n, dt

    def nonlinear(self, w, g):
        inv = lambda f: torch.fft.irfft2(f, s=(self.n, self.n))
        psi = w * self.ik2
        u, v = inv(1j * self.ky * psi), inv(-1j * self.kx * psi)
        return -self.M * torch.fft.rfft2(u * inv(1j * self.kx * w) + v * inv(1j * self.ky * w)) + g

    def advance(self, wf, gf, nsteps):
        w, g, dt, E, E2 = self.M * torch.fft.rfft2(wf), self.M * torch.fft.rfft2(gf), self.dt, self.E, self.E2
        for _ in range(nsteps):
            a = self.nonlinear(w, g)
            b = self.nonlinear(E * (w + dt / 2 * a), g)
            c = self.nonlinear(E * w + dt / 2 * b, g)
            d = self.nonlinear(E2 * w + dt * E * c, g)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
        return torch.fft.irfft2(w, s=(self.n, self.n))


def timing(args):
    out = []
    parent = parent_steps(args.parent_lib) if args.parent_lib else None
    for n, B in CASES:
        s = PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG).kolmogorov_forcing(4, 1.0)
        plain = PeriodicSolver(n, n, DT, 1.0, NU)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        st = s.init(dev(u0), dev(v0))
        s.step(st, 20)                                                    # a developed state
        saved = st.clone()
        w0 = s.vorticity(st)
        g = s.vorticity(PeriodicState(s.ghat, torch.zeros((1, 2), device='cuda'), torch.empty(0, dtype=torch.uint8, device='cuda')))   # the force as a field
        r = dev(O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0)[0])
        steps = args.steps
        what0 = torch.empty((steps,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        lam0 = s.init_vorticity(r).what
        lam, gbar = lam0.clone(), torch.empty_like(lam0)
        awork = torch.empty(ops.spec_ns_adjoint_workspace(B, n, n), dtype=torch.uint8, device='cuda')

        def restore():
            st.what.copy_(saved.what)

        def fwd_keep():
            for k in range(steps):
                what0[k].copy_(st.what)
                ops.spec_ns_step_forced_(st.what, st.mean, s.ghat, st.work, n, s.Lx, s.Ly, s.dt, s.nu, s.drag, 1)

        def adjoint():
            lam.copy_(lam0)
            ops.spec_ns_step_adjoint_(what0, st.mean, s.ghat, lam, gbar, awork, n, s.Lx, s.Ly, s.dt, s.nu, s.drag)

        def autograd():
            a, f = w0.detach().requires_grad_(True), g.detach().requires_grad_(True)
            (s.advance(a, steps, mean=st.mean, forcing=f) * r).sum().backward()

        variants = [('forward_step', lambda: s.step(st, steps)), ('forward_keeping_starts', fwd_keep), ('adjoint_call', adjoint),
                    ('advance_forward_backward', autograd)]
        if not args.no_torch:
            T = TorchScheme(n, DT, NU, DRAG)

            def torch_autograd():
                a, f = w0.detach().requires_grad_(True), g.detach().requires_grad_(True)
                (T.advance(a, f, steps) * r).sum().backward()
            variants.append(('torch_fft_autograd_forward_backward', torch_autograd))
        case = dict(nx=n, ny=n, batch=B, kept_bytes_per_step=int(8 * B * s.my1 * n))
        if parent:
            variants.append(('forward_step_parent_lib', lambda: parent['forced'](s, st, steps)))
            variants.append(('unforced_step', lambda: plain.step(st, steps)))
            variants.append(('unforced_step_parent_lib', lambda: parent['unforced'](plain, st, steps)))
            for name, sol in (('forced', s), ('unforced', plain)):
                restore()
                sol.step(st, 3)
                mine = st.what.clone()
                restore()
                parent[name](sol, st, 3)
                case[name + '_bitwise_parent_lib'] = bool(torch.equal(mine, st.what))
        restore()
        fwd_keep()                                                        # what0 for the adjoint's warm-up
        for _, fn in variants:
            restore()
            fn()
        torch.cuda.synchronize()
        ts = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                restore()
                torch.cuda.synchronize()
                ts[name].append(event_ms(fn))
        for name, _ in variants:
            case[name] = stats(ts[name], steps)
        case['adjoint_over_forward'] = ratio(ts['adjoint_call'], ts['forward_step'])
        case['advance_forward_backward_over_forward'] = ratio(ts['advance_forward_backward'], ts['forward_step'])
        case['keeping_starts_over_forward'] = ratio(ts['forward_keeping_starts'], ts['forward_step'])
        if not args.no_torch:
            case['torch_over_advance'] = ratio(ts['torch_fft_autograd_forward_backward'], ts['advance_forward_backward'])
        if parent:
            case['forced_over_parent_lib'] = ratio(ts['forward_step'], ts['forward_step_parent_lib'])
            case['unforced_over_parent_lib'] = ratio(ts['unforced_step'], ts['unforced_step_parent_lib'])
        case['model_adjoint_over_forward'] = 2.6
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, saved, what0, awork
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_adjoint_cases as AC
    cplx = lambda t: t.cpu().numpy().astype(np.float64)[..., 0] + 1j * t.cpu().numpy().astype(np.float64)[..., 1]
    rows = []
    for c in AC.CASES:
        nx, ny, B, Lx, Ly, mean = c
        d = AC.inputs(c)
        s = PeriodicSolver(nx, ny, d['dt'], AC.RHO, AC.NU, Lx=Lx, Ly=Ly, drag=AC.DRAG)
        ghat = s.init(dev(d['fx']), dev(d['fy'])).what
        st = s.init(dev(d['u0']), dev(d['v0']))
        what0 = torch.empty((AC.NSTEPS,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        for k in range(AC.NSTEPS):
            what0[k].copy_(st.what)
            ops.spec_ns_step_forced_(st.what, st.mean, ghat, st.work, ny, Lx, Ly, s.dt, s.nu, s.drag, 1)
        lam = s.init_vorticity(dev(d['r'])).what
        gbar = torch.empty_like(lam)
        work = torch.empty(ops.spec_ns_adjoint_workspace(B, nx, ny), dtype=torch.uint8, device='cuda')
        ops.spec_ns_step_adjoint_(what0, st.mean, ghat, lam, gbar, work, ny, Lx, Ly, s.dt, s.nu, s.drag)
        rw, rg = AC.oracle_gradient(c)
        row = dict(case=AC.case_id(c), steps=AC.NSTEPS, wbar=float('%.3e' % AC.rel(cplx(lam), rw)), gbar=float('%.3e' % AC.rel(cplx(gbar), rg)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(gradients=rows, bound=AC.BOUND)


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the adjoint and stage-keeping kernels from the text of `llvm-readelf --notes` on the library."""
    if not path or not os.path.exists(path):
        return None
    txt = open(path).read()
    res = {}
    for blk in txt.split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and ('ps_row_adj' in name.group(1) or 'ps_col_adj' in name.group(1) or 'PsKeep' in name.group(1)):
            res[name.group(1)] = dict(vgprs=int(vg.group(1)), scratch_bytes=int(sc.group(1)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=20, help='steps per timing')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's) for the same-process A/B")
    ap.add_argument('--isa-notes', default=None, help='text of llvm-readelf --notes on libnns_hip.so (registers and scratch per kernel)')
    ap.add_argument('--no-accuracy', action='store_true')
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps)
    if not args.no_accuracy:
        rec['accuracy'] = accuracy()
    rec['timing'] = timing(args)
    rec['kernels'] = kernel_resources(args.isa_notes)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_adjoint_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
