"""Measures the periodic spectral solver's reverse mode in its linear operator (nns.periodic.PeriodicSolver.evolve with ``operator``:
nns_spec_ns_step_operator_adjoint_f32 of csrc/pspec_kernels.hip).  Writes ONE JSON record to OUTDIR/pspec_operator_grad_run.json and prints it.

    python tools/pspec_operator_grad_run.py OUTDIR [--steps 20] [--reps 7] [--commit ID] [--parent-lib PATH] [--name NAME] [--isa-notes FILE] [--no-accuracy] [--no-torch]

Timing: at 256^2 x 64 and 1024^2 x 8 (the states, forces and linear terms of tools/pspec_linear_adjoint_run.py) these take turns within every
repetition, each on the same saved start spectra: the linear adjoint call without and with lbar, for the flow and for the buoyant scalar;
forward + backward through ``evolve`` with the solver's own table, the same table passed as a constant ``operator`` and as one that requires
grad; and, unless --no-torch, forward + backward of the same scheme composed from torch.fft ops with the table as a leaf.  With --parent-lib
also whether the linear adjoint of another build of the library (the parent commit's) loaded into the same process gives the same bits, and
this build's call against the parent's in the same rotation, each twice (this, parent, parent, this): the ratio of the parent's two turns is
the noise the A/B ratio is read against.  A timing is device events around the work, reported per step as the median over the repetitions
with the spread (max - min) / median; ratios are medians of the per-repetition ratios.

What to compare against: the byte model.  The flow's adjoint moves 132 compact fields per step; the table's cotangent adds five reads (s3, w0,
s2, w0, s1) and three reads and three writes of the two sums: 11, so 143 / 132 = 1.083x.  The scalar's adjoint moves 219: 230 / 219 = 1.050x.
Accuracy (tests/pspec_operator_grad_cases.py, the figures tests/test_gpu_pspec_operator_grad.py bounds): the table's gradient after 3 steps
against the float64 restatement, in rel-L2 over the table.  The register and scratch figures of the new kernels come from the code object's
metadata (--isa-notes FILE: the text of `llvm-readelf --notes` on the library, or the amdhsa.kernels block that ends the listing of
tools/isa_listing.py)."""
import argparse
import ctypes
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import torch  # noqa: E402

import pspec_oracle as O  # noqa: E402
from nns import _lib, ops  # noqa: E402
from nns.periodic import PeriodicSolver, PeriodicState  # noqa: E402
from pspec_adjoint_run import event_ms, stats, ratio, dev, TorchScheme  # noqa: E402
from pspec_linear_run import linear_kw  # noqa: E402

CASES = [(256, 64), (1024, 8)]
DT, NU, DRAG, KAPPA, GRAD, BUOY = 1e-3, 1e-3, 0.1, 1e-3, (0.0, 1.0), (0.0, 1.0)
MODEL = dict(flow=round(143 / 132, 4), scalar=round(230 / 219, 4))     # compact fields moved per step with / without lbar


def linear_adjoint_of(path):
    """nns_spec_ns_step_linear_adjoint_f32 of a build of the library, through its own ctypes handle, for the flow (no scalar)."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_linear_adjoint_f32.argtypes = [P] * 4 + [I] + [P] * 4 + [Z] + [I] * 3 + [D] * 8 + [P, I, P]
    p = lambda t: t.data_ptr()

    def call(s, what0, mean, lam, gbar, work, lin):
        rc = L.nns_spec_ns_step_linear_adjoint_f32(p(what0), None, p(mean), p(s.ghat), 1, p(lam), None, p(gbar), p(work), work.numel(), lam.shape[0],
                                                   s.nx, s.ny, s.Lx, s.Ly, s.dt, 0.0, 0.0, 0.0, 0.0, 0.0, p(lin), what0.shape[0],
                                                   torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('the library %s refused the call: %d' % (path, rc))
    return call


class TorchTableScheme(TorchScheme):
    """TorchScheme with its factors made from a table leaf [n, n // 2 + 1, 2] = (Re, Im)(lambda dt / 2) inside the graph."""

    def advance_table(self, wf, gf, nsteps, table):
        l = torch.view_as_complex(table)
        self.E, self.E2 = torch.exp(l), torch.exp(2 * l)
        return self.advance(wf, gf, nsteps)


def timing(args):
    out = []
    for n, B in CASES:
        mk = lambda **kw: PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, **kw).kolmogorov_forcing(4, 1.0)
        sc = dict(kappa=KAPPA, scalar_gradient=GRAD, buoyancy=BUOY)
        linear, linear_sc = mk(**linear_kw(n)), mk(**sc, **linear_kw(n))
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 1, umax=1.0)[0]
        st = linear_sc.init(dev(u0), dev(v0), dev(th0))
        linear_sc.step(st, 20)                                            # a developed state
        sf = PeriodicState(st.what, st.mean, st.work)                     # the same buffers without the scalar
        w0 = linear.vorticity(sf)
        g = linear.vorticity(PeriodicState(linear.ghat, torch.zeros((1, 2), device='cuda'), torch.empty(0, dtype=torch.uint8, device='cuda')))
        rw, rt = (dev(f) for f in O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0))
        steps = args.steps
        what0 = torch.empty((steps,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        that0 = torch.empty_like(what0)
        for k in range(steps):
            what0[k].copy_(st.what)
            that0[k].copy_(st.that)
            linear_sc.step(st, 1)
        lam0 = linear.init_vorticity(rw).what
        mu0 = linear_sc.init(torch.zeros_like(rt), torch.zeros_like(rt), rt).that
        lam, mu, gbar, lbar = lam0.clone(), mu0.clone(), torch.empty_like(lam0), torch.empty_like(lam0)
        awork = torch.empty(ops.spec_ns_scalar_adjoint_workspace(B, n, n), dtype=torch.uint8, device='cuda')
        lin = linear._linear_of(st)
        box = (n, linear.Lx, linear.Ly, DT)

        def adjoint(s, scalar, table_grad):
            lam.copy_(lam0)
            mu.copy_(mu0)
            ops.spec_ns_step_operator_adjoint_(what0, that0 if scalar else None, st.mean, s.ghat, lam, mu if scalar else None, gbar, awork, *box,
                                               KAPPA, GRAD, BUOY, lin, lbar if table_grad else None)

        def autograd(operator):
            a, f = (x.detach().requires_grad_(True) for x in (w0, g))
            (linear.evolve(a, steps, mean=st.mean, forcing=f, operator=operator) * rw).sum().backward()

        variants = [('linear_adjoint_call', lambda: adjoint(linear, False, False)), ('operator_adjoint_call', lambda: adjoint(linear, False, True)),
                    ('linear_scalar_adjoint_call', lambda: adjoint(linear_sc, True, False)),
                    ('operator_scalar_adjoint_call', lambda: adjoint(linear_sc, True, True)),
                    ('evolve_forward_backward', lambda: autograd(None)),
                    ('evolve_constant_operator_forward_backward', lambda: autograd(lin)),
                    ('evolve_operator_grad_forward_backward', lambda: autograd(lin.clone().requires_grad_(True)))]
        case = dict(nx=n, ny=n, batch=B, table_bytes=int(8 * linear.my1 * n), lbar_bytes=int(8 * B * linear.my1 * n))
        if not args.no_torch:
            ts_ = TorchTableScheme(n, DT, NU, DRAG)
            full = torch.zeros((n, n // 2 + 1, 2), device='cuda')
            full[:, :linear.my1] = lin.transpose(0, 1)

            def torch_autograd():
                a, f, t = (x.detach().requires_grad_(True) for x in (w0, g, full))
                (ts_.advance_table(a, f, steps, t) * rw).sum().backward()
            variants.append(('torch_fft_operator_grad_forward_backward', torch_autograd))
        if args.parent_lib:
            this, parent = linear_adjoint_of(_lib.LIB_PATH), linear_adjoint_of(args.parent_lib)
            lam.copy_(lam0)
            this(linear, what0, st.mean, lam, gbar, awork, lin)
            mine = (lam.clone(), gbar.clone())
            lam.copy_(lam0)
            parent(linear, what0, st.mean, lam, gbar, awork, lin)
            case['linear_adjoint_bitwise_parent_lib'] = bool(torch.equal(mine[0], lam) and torch.equal(mine[1], gbar))
            for tag, call in (('', this), ('_parent_lib', parent), ('_parent_lib_again', parent), ('_again', this)):
                def direct(call=call):
                    lam.copy_(lam0)
                    call(linear, what0, st.mean, lam, gbar, awork, lin)
                variants.append(('linear_adjoint_direct' + tag, direct))
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        ts = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                torch.cuda.synchronize()
                ts[name].append(event_ms(fn))
        for name, _ in variants:
            case[name] = stats(ts[name], steps)
        r = lambda a, b: ratio(ts[a], ts[b])
        case['operator_over_linear_adjoint'] = r('operator_adjoint_call', 'linear_adjoint_call')
        case['operator_over_linear_scalar_adjoint'] = r('operator_scalar_adjoint_call', 'linear_scalar_adjoint_call')
        case['byte_model'] = MODEL
        case['evolve_constant_operator_over_evolve'] = r('evolve_constant_operator_forward_backward', 'evolve_forward_backward')
        case['evolve_operator_grad_over_evolve'] = r('evolve_operator_grad_forward_backward', 'evolve_forward_backward')
        if not args.no_torch:
            case['torch_fft_over_evolve_operator_grad'] = r('torch_fft_operator_grad_forward_backward', 'evolve_operator_grad_forward_backward')
        if args.parent_lib:
            what = 'linear_adjoint_direct'
            ab, aa = r(what, what + '_parent_lib'), r(what + '_parent_lib_again', what + '_parent_lib')
            case[what + '_over_parent_lib'], case[what + '_parent_lib_again_over_parent_lib'] = ab, aa
            case[what + '_median_inside_parent_lib_noise'] = bool(aa['min'] <= ab['median'] <= aa['max'])
            case[what + '_again_over_parent_lib'] = r(what + '_again', what + '_parent_lib')
            case[what + '_again_over_first_turn'] = r(what + '_again', what)
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, sf, what0, that0, awork
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_operator_grad_cases as OC
    cplx = lambda t: t.cpu().numpy().astype(np.float64)[..., 0] + 1j * t.cpu().numpy().astype(np.float64)[..., 1]
    rows = []
    for kind, c in OC.RUNS:
        nx, ny, B, Lx, Ly, _ = c
        d = OC.inputs(c)
        s = OC.LA.solver(kind, c, d['dt'])
        scalar = kind in ('scalar', 'buoyant')
        ghat = s.init(dev(d['fx']), dev(d['fy'])).what
        st = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']) if scalar else None)
        what0 = torch.empty((OC.NSTEPS,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        that0 = torch.empty_like(what0) if scalar else None
        s.ghat = ghat
        for k in range(OC.NSTEPS):
            what0[k].copy_(st.what)
            if scalar:
                that0[k].copy_(st.that)
            s.step(st, 1)
        lam = s.init_vorticity(dev(d['rw'])).what
        z = torch.zeros((B, nx, ny), device='cuda')
        mu = s.init(z, z, dev(d['rt'])).that if scalar else None
        lbar = torch.empty_like(lam)
        size = ops.spec_ns_scalar_adjoint_workspace if scalar else ops.spec_ns_adjoint_workspace
        work = torch.empty(size(B, nx, ny), dtype=torch.uint8, device='cuda')
        ops.spec_ns_step_operator_adjoint_(what0, that0, st.mean, ghat, lam, mu, None, work, ny, Lx, Ly, s.dt, s.kappa if scalar else 0.0,
                                           s.scalar_gradient, s.buoyancy, s._linear_of(st), lbar)
        err = float('%.3e' % OC.rel(cplx(s._operator_gradient(lbar)), OC.table_gradient(kind, c)))
        row = dict(run=OC.run_id((kind, c)), steps=OC.NSTEPS, bound=OC.bound(kind), table_gradient=err)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(gradients=rows, bound_flow=OC.BOUND_FLOW, bound_scalar=OC.BOUND_SCALAR)


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the operator adjoint kernels from the text of `llvm-readelf --notes`."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and re.search(r'PsAdj(Scalar)?Operator', name.group(1)):
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
    ap.add_argument('--name', default='pspec_operator_grad_run', help='the record is OUTDIR/NAME.json')
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
