"""Measures the reverse mode of the periodic spectral solver's scalar and buoyant step (nns.periodic.PeriodicSolver.advance_scalar:
nns_spec_ns_step_scalar_adjoint_f32 of csrc/pspec_kernels.hip).  Writes ONE JSON record to OUTDIR/pspec_scalar_adjoint_run.json and prints it.

    python tools/pspec_scalar_adjoint_run.py OUTDIR [--steps 20] [--reps 7] [--commit ID] [--parent-lib PATH] [--name NAME] [--isa-notes FILE] [--no-accuracy] [--no-torch]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow and scalar, Kolmogorov force k = 4, drag 0.1, kappa = nu, G = (0, 1); buoyant: b = (0, 1))
these take turns within every repetition, each from the same saved state: the flow's forced step and its adjoint call (the parent's kernels,
in this process), then for the passive and for the buoyant scalar the forward step, the adjoint call alone and forward + backward through
``advance_scalar`` (autograd, a differentiable forcing) and, unless --no-torch, forward + backward of the buoyant scheme composed from torch.fft
ops in float32 under torch autograd.  With --parent-lib also whether the forward steps and the flow's adjoint of another build of the library
(the parent commit's) loaded into the same process give the same bits, and the flow's adjoint call of this build against the parent's in the
same rotation, the parent's twice: the ratio of its two turns is the noise the A/B ratio is read against.  A timing is device events around the work, reported per step as the
median over the repetitions with the spread (max - min) / median; ratios are medians of the per-repetition ratios.

The byte model to compare against, in compacted fields c moved per step (DESIGN.md section 4.2 has the count): the flow's adjoint 132c, the
scalar's 219c, so 1.66x the flow's adjoint and 2.49x the forced scalar step's 88c.
Accuracy (tests/pspec_scalar_adjoint_cases.py, the figures tests/test_gpu_pspec_scalar_adjoint.py bounds): wbar, thetabar and gbar after 3 steps
against the float64 restatement.  The register and scratch figures of the new kernels come from the code object's metadata (--isa-notes FILE:
the text of `llvm-readelf --notes` on the library, or the amdhsa.kernels block that ends the listing of tools/isa_listing.py, made at build
time)."""
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
from nns import _lib, ops  # noqa: E402
from nns.periodic import PeriodicSolver, PeriodicState  # noqa: E402
from pspec_adjoint_run import event_ms, stats, ratio, dev  # noqa: E402

CASES = [(256, 64), (1024, 8)]
DT, NU, DRAG, KAPPA, GRAD, BUOY = 1e-3, 1e-3, 0.1, 1e-3, (0.0, 1.0), (0.0, 1.0)
MODEL_C = dict(flow_adjoint=132, scalar_adjoint=219, scalar_step=88)


class TorchBuoyantScheme(object):
    """The same Lawson RK4 scheme of (w, theta) from torch.fft ops in float32, for torch autograd (the comparison, not the product)."""

    def __init__(self, n, dt, nu, drag, kappa, grad, buoy):
        m = torch.fft.fftfreq(n, 1.0 / n, device='cuda')
        j = torch.arange(n // 2 + 1, device='cuda', dtype=torch.float32)
        self.kx, self.ky = m[:, None], j[None, :]
        k2 = self.kx ** 2 + self.ky ** 2
        self.Mt = ((3 * m.abs()[:, None] < n) & (3 * j[None, :] < n)).float()
        self.M = self.Mt * (k2 > 0).float()
        self.ik2 = torch.where(k2 > 0, 1.0 / torch.where(k2 > 0, k2, torch.ones_like(k2)), torch.zeros_like(k2))
        self.E, self.E2 = torch.exp(-(nu * k2 + drag) * dt / 2), torch.exp(-(nu * k2 + drag) * dt)
        self.Et, self.Et2 = torch.exp(-kappa * k2 * dt / 2), torch.exp(-kappa * k2 * dt)
        self.n, self.dt, self.grad, self.buoy = n, dt, grad, buoy

    def nonlinear(self, w, t, g):
        inv = lambda f: torch.fft.irfft2(f, s=(self.n, self.n))
        psi = w * self.ik2
        u, v = inv(1j * self.ky * psi), inv(-1j * self.kx * psi)
        nw = -self.M * torch.fft.rfft2(u * inv(1j * self.kx * w) + v * inv(1j * self.ky * w)) + g
        nw = nw + self.M * (1j * self.kx * self.buoy[1] - 1j * self.ky * self.buoy[0]) * t
        nt = -self.Mt * torch.fft.rfft2(u * (inv(1j * self.kx * t) + self.grad[0]) + v * (inv(1j * self.ky * t) + self.grad[1]))
        return nw, nt

    def advance(self, wf, tf, gf, nsteps):
        w, t, g = self.M * torch.fft.rfft2(wf), self.Mt * torch.fft.rfft2(tf), self.M * torch.fft.rfft2(gf)
        dt, E, E2, Et, Et2 = self.dt, self.E, self.E2, self.Et, self.Et2
        for _ in range(nsteps):
            a, at = self.nonlinear(w, t, g)
            b, bt = self.nonlinear(E * (w + dt / 2 * a), Et * (t + dt / 2 * at), g)
            c, ct = self.nonlinear(E * w + dt / 2 * b, Et * t + dt / 2 * bt, g)
            d, dth = self.nonlinear(E2 * w + dt * E * c, Et2 * t + dt * Et * ct, g)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
            t = Et2 * t + dt / 6 * (Et2 * at + 2 * Et * (bt + ct) + dth)
        return torch.fft.irfft2(w, s=(self.n, self.n)), torch.fft.irfft2(t, s=(self.n, self.n))


def parent_calls(path):
    """The parent library's forward steps and flow adjoint, under the argument lists of include/nns.h."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_forced_f32.argtypes = [P] * 3 + [I, P, Z] + [I] * 3 + [D] * 5 + [I, P]
    L.nns_spec_ns_step_buoyant_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 10 + [I, P]
    L.nns_spec_ns_step_adjoint_f32.argtypes = [P] * 3 + [I, P, P, P, Z] + [I] * 3 + [D] * 5 + [I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def check(rc):
        if rc != 0:
            raise RuntimeError('the parent library refused the call: %d' % rc)

    def forced(s, st, n):
        check(L.nns_spec_ns_step_forced_f32(p(st.what), p(st.mean), p(s.ghat), 1, p(st.work), st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly,
                                            s.dt, s.nu, s.drag, n, stream()))

    def buoyant(s, st, n):                                                # b = (0, 0) makes the passive scalar's calls
        check(L.nns_spec_ns_step_buoyant_f32(p(st.what), p(st.that), p(st.mean), p(s.ghat), 1, p(st.work), st.work.numel(), st.batch, s.nx, s.ny,
                                             s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient[0], s.scalar_gradient[1], s.buoyancy[0],
                                             s.buoyancy[1], n, stream()))

    def adjoint(s, what0, mean, lam, gbar, work):
        check(L.nns_spec_ns_step_adjoint_f32(p(what0), p(mean), p(s.ghat), 1, p(lam), p(gbar), p(work), work.numel(), lam.shape[0], s.nx, s.ny, s.Lx,
                                             s.Ly, s.dt, s.nu, s.drag, what0.shape[0], stream()))
    L.nns_spec_ns_step_scalar_adjoint_f32.argtypes = [P] * 4 + [I] + [P] * 4 + [Z] + [I] * 3 + [D] * 10 + [I, P]

    def scalar_adjoint(s, what0, that0, mean, lam, mu, gbar, work):
        check(L.nns_spec_ns_step_scalar_adjoint_f32(p(what0), p(that0), p(mean), p(s.ghat), 1, p(lam), p(mu), p(gbar), p(work), work.numel(),
                                                    lam.shape[0], s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient[0],
                                                    s.scalar_gradient[1], s.buoyancy[0], s.buoyancy[1], what0.shape[0], stream()))
    return dict(forced=forced, buoyant=buoyant, adjoint=adjoint, scalar_adjoint=scalar_adjoint)


def timing(args):
    out = []
    parent = parent_calls(args.parent_lib) if args.parent_lib else None
    for n, B in CASES:
        mk = lambda **kw: PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, **kw).kolmogorov_forcing(4, 1.0)
        flow = mk()
        sol = dict(passive=mk(kappa=KAPPA, scalar_gradient=GRAD), buoyant=mk(kappa=KAPPA, scalar_gradient=GRAD, buoyancy=BUOY))
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 1, umax=1.0)[0]
        st = sol['buoyant'].init(dev(u0), dev(v0), dev(th0))
        sol['buoyant'].step(st, 20)                                       # a developed state
        saved = st.clone()
        w0, t0 = sol['buoyant'].vorticity(st), sol['buoyant'].scalar(st)
        g = flow.vorticity(PeriodicState(flow.ghat, torch.zeros((1, 2), device='cuda'), torch.empty(0, dtype=torch.uint8, device='cuda')))   # the force as a field
        rw, rt = (dev(f) for f in O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0))
        steps = args.steps
        what0 = torch.empty((steps,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        that0 = torch.empty_like(what0)
        lam0 = flow.init_vorticity(rw).what
        mu0 = sol['passive'].init(torch.zeros_like(rt), torch.zeros_like(rt), rt).that
        lam, mu, gbar = lam0.clone(), mu0.clone(), torch.empty_like(lam0)
        awork = torch.empty(ops.spec_ns_scalar_adjoint_workspace(B, n, n), dtype=torch.uint8, device='cuda')

        def restore():
            st.what.copy_(saved.what)
            st.that.copy_(saved.that)

        def keep(s):
            box = (st.mean, s.ghat, st.work, n, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient, s.buoyancy)
            for k in range(steps):
                what0[k].copy_(st.what)
                that0[k].copy_(st.that)
                ops.spec_ns_step_buoyant_(st.what, st.that, *box, 1)

        def flow_step():
            ops.spec_ns_step_forced_(st.what, st.mean, flow.ghat, st.work, n, flow.Lx, flow.Ly, flow.dt, flow.nu, flow.drag, steps)

        def flow_adjoint():
            lam.copy_(lam0)
            ops.spec_ns_step_adjoint_(what0, st.mean, flow.ghat, lam, gbar, awork, n, flow.Lx, flow.Ly, flow.dt, flow.nu, flow.drag)

        def adjoint(s):
            lam.copy_(lam0)
            mu.copy_(mu0)
            ops.spec_ns_step_scalar_adjoint_(what0, that0, st.mean, s.ghat, lam, mu, gbar, awork, n, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa,
                                             s.scalar_gradient, s.buoyancy)

        def autograd(s):
            a, t, f = (x.detach().requires_grad_(True) for x in (w0, t0, g))
            ow, ot = s.advance_scalar(a, t, steps, mean=st.mean, forcing=f)
            ((ow * rw).sum() + (ot * rt).sum()).backward()

        variants = [('flow_step', flow_step), ('flow_adjoint_call', flow_adjoint)]
        for kind in ('passive', 'buoyant'):
            s = sol[kind]
            variants += [(kind + '_step', lambda s=s: s.step(st, steps)), (kind + '_adjoint_call', lambda s=s: adjoint(s)),
                         (kind + '_advance_forward_backward', lambda s=s: autograd(s))]
        if not args.no_torch:
            T = TorchBuoyantScheme(n, DT, NU, DRAG, KAPPA, GRAD, BUOY)

            def torch_autograd():
                a, t, f = (x.detach().requires_grad_(True) for x in (w0, t0, g))
                ow, ot = T.advance(a, t, f, steps)
                ((ow * rw).sum() + (ot * rt).sum()).backward()
            variants.append(('torch_fft_autograd_forward_backward', torch_autograd))
        case = dict(nx=n, ny=n, batch=B, kept_bytes_per_step=int(16 * B * flow.my1 * n))
        restore()
        keep(sol['buoyant'])                                              # what0, that0 for the adjoint calls
        if parent:
            for name, s in (('forced', flow), ('passive', sol['passive']), ('buoyant', sol['buoyant'])):
                restore()
                s.step(st, 3) if name != 'forced' else ops.spec_ns_step_forced_(st.what, st.mean, s.ghat, st.work, n, s.Lx, s.Ly, s.dt, s.nu, s.drag, 3)
                mine = (st.what.clone(), st.that.clone())
                restore()
                parent['forced' if name == 'forced' else 'buoyant'](s, st, 3)
                case[name + '_step_bitwise_parent_lib'] = bool(torch.equal(mine[0], st.what) and torch.equal(mine[1], st.that))
            flow_adjoint()
            mine = (lam.clone(), gbar.clone())
            lam.copy_(lam0)
            parent['adjoint'](flow, what0, st.mean, lam, gbar, awork)
            case['flow_adjoint_bitwise_parent_lib'] = bool(torch.equal(mine[0], lam) and torch.equal(mine[1], gbar))
            for kind in ('passive', 'buoyant'):
                adjoint(sol[kind])
                mine = (lam.clone(), mu.clone(), gbar.clone())
                lam.copy_(lam0)
                mu.copy_(mu0)
                parent['scalar_adjoint'](sol[kind], what0, that0, st.mean, lam, mu, gbar, awork)
                case[kind + '_adjoint_bitwise_parent_lib'] = bool(all(torch.equal(a, b) for a, b in zip(mine, (lam, mu, gbar))))
            # the flow's adjoint of this build and of the parent's under the same direct call, the parent's twice: the A/A ratio is the noise
            this = parent_calls(_lib.LIB_PATH)
            for name, calls in (('flow_adjoint_direct', this), ('flow_adjoint_direct_parent_lib', parent), ('flow_adjoint_direct_parent_lib_again', parent)):
                def direct(calls=calls):
                    lam.copy_(lam0)
                    calls['adjoint'](flow, what0, st.mean, lam, gbar, awork)
                variants.insert(2, (name, direct))
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
        case['flow_adjoint_over_flow_step'] = ratio(ts['flow_adjoint_call'], ts['flow_step'])
        if parent:
            ab = ratio(ts['flow_adjoint_direct'], ts['flow_adjoint_direct_parent_lib'])
            aa = ratio(ts['flow_adjoint_direct_parent_lib_again'], ts['flow_adjoint_direct_parent_lib'])
            case['flow_adjoint_over_parent_lib'], case['parent_lib_again_over_parent_lib'] = ab, aa
            case['flow_adjoint_median_inside_parent_lib_noise'] = bool(aa['min'] <= ab['median'] <= aa['max'])
        for kind in ('passive', 'buoyant'):
            case[kind + '_adjoint_over_step'] = ratio(ts[kind + '_adjoint_call'], ts[kind + '_step'])
            case[kind + '_adjoint_over_flow_adjoint'] = ratio(ts[kind + '_adjoint_call'], ts['flow_adjoint_call'])
            case[kind + '_advance_forward_backward_over_step'] = ratio(ts[kind + '_advance_forward_backward'], ts[kind + '_step'])
        if not args.no_torch:
            case['torch_over_buoyant_advance'] = ratio(ts['torch_fft_autograd_forward_backward'], ts['buoyant_advance_forward_backward'])
        case['model_bytes_in_compacted_fields'] = MODEL_C
        case['model_adjoint_over_flow_adjoint'] = round(MODEL_C['scalar_adjoint'] / MODEL_C['flow_adjoint'], 3)
        case['model_adjoint_over_step'] = round(MODEL_C['scalar_adjoint'] / MODEL_C['scalar_step'], 3)
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, saved, what0, that0, awork
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_scalar_adjoint_cases as AC
    cplx = lambda t: t.cpu().numpy().astype(np.float64)[..., 0] + 1j * t.cpu().numpy().astype(np.float64)[..., 1]
    rows = []
    for c in AC.CASES:
        nx, ny, B, Lx, Ly, mean, buoy = c
        d = AC.inputs(c)
        s = PeriodicSolver(nx, ny, d['dt'], AC.RHO, AC.NU, Lx=Lx, Ly=Ly, drag=AC.DRAG, kappa=AC.KAPPA, scalar_gradient=AC.GRAD, buoyancy=buoy)
        ghat = s.init(dev(d['fx']), dev(d['fy'])).what
        st = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']))
        what0 = torch.empty((AC.NSTEPS,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        that0 = torch.empty_like(what0)
        for k in range(AC.NSTEPS):
            what0[k].copy_(st.what)
            that0[k].copy_(st.that)
            ops.spec_ns_step_buoyant_(st.what, st.that, st.mean, ghat, st.work, ny, Lx, Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient, buoy, 1)
        lam = s.init_vorticity(dev(d['rw'])).what
        z = torch.zeros((B, nx, ny), device='cuda')
        mu = s.init(z, z, dev(d['rt'])).that
        gbar = torch.empty_like(lam)
        work = torch.empty(ops.spec_ns_scalar_adjoint_workspace(B, nx, ny), dtype=torch.uint8, device='cuda')
        ops.spec_ns_step_scalar_adjoint_(what0, that0, st.mean, ghat, lam, mu, gbar, work, ny, Lx, Ly, s.dt, s.nu, s.drag, s.kappa,
                                         s.scalar_gradient, buoy)
        errs = [float('%.3e' % AC.rel(cplx(g), r)) for g, r in zip((lam, mu, gbar), AC.oracle_gradient(c))]
        row = dict(case=AC.case_id(c), steps=AC.NSTEPS, wbar=errs[0], thetabar=errs[1], gbar=errs[2])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(gradients=rows, bound=AC.BOUND)


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the scalar adjoint and stage-keeping kernels from the text of `llvm-readelf --notes` on the library."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and any(k in name.group(1) for k in ('PsAdjScalar', 'PsAdjGrad', 'PsKeepScalar')):
            res[name.group(1)] = dict(vgprs=int(vg.group(1)), scratch_bytes=int(sc.group(1)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=20, help='steps per timing')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's) for the same-process comparison")
    ap.add_argument('--isa-notes', default=None, help='text of llvm-readelf --notes on libnns_hip.so (registers and scratch per kernel)')
    ap.add_argument('--name', default='pspec_scalar_adjoint_run', help='the record is OUTDIR/NAME.json')
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
    with open(os.path.join(args.outdir, args.name + '.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
