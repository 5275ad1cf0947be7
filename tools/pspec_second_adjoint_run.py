"""Measures the second-order adjoint of the periodic spectral solver's step (nns.periodic.PeriodicSolver.second_order_forward /
hessian_vector_product: nns_spec_ns_step_second_adjoint_f32 of csrc/pspec_kernels.hip, kernels in csrc/pspec_second_adjoint.hip).  Writes ONE
JSON record to OUTDIR/pspec_second_adjoint_run.json and prints it.

    python tools/pspec_second_adjoint_run.py OUTDIR [--steps 10] [--reps 7] [--commit ID] [--parent-lib PATH] [--isa-listing FILE] [--no-accuracy]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow, perturbation and cotangents, Kolmogorov force k = 4, drag 0.1) these take turns within
every repetition, on the start spectra one tangent forward saved: the second-order adjoint, the first-order adjoint and the tangent step of
this build and, with --parent-lib, the first-order adjoint and the tangent step of another build of the library (the parent commit's) under
the same direct call, the parent's twice with this build's turn between them: the ratio of the parent's two turns is the noise the A/B ratio
is read against; also whether both builds give the same bits.  Then the whole product, ``second_order_forward`` + ``backward``, against the
finite-difference alternative it replaces: two forward + backward passes of ``evolve``.  A timing is device events around the work, reported
per step as the median over the repetitions with the spread (max - min) / median; ratios are medians of the per-repetition ratios.

The byte model to compare against, in compacted fields c moved per step: the flow's step 50c, the tangent's 100c, the
adjoint's 132c, the second-order adjoint's 264c; the whole product 100c + 264c = 364c, the finite difference 2 (50c + 132c) = 364c.
Accuracy (tests/pspec_second_adjoint_cases.py, the figures tests/test_gpu_pspec_second_adjoint.py bounds): dwbar and dgbar after 3 steps
against the float64 restatement in both settings, and the symmetry of the Hessian.  The register and scratch figures of the new kernels come
from the listing of tools/isa_listing.py (--isa-listing: pspec_second_adjoint.s)."""
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
from nns.periodic import PeriodicSolver  # noqa: E402
from pspec_adjoint_run import event_ms, stats, ratio, dev  # noqa: E402

CASES = [(256, 64), (1024, 8)]
DT, NU, DRAG = 1e-3, 1e-3, 0.1
MODEL_C = dict(flow_step=50, tangent_step=100, adjoint=132, second_adjoint=264, product=364, finite_difference=364)


def direct_calls(path):
    """The first-order adjoint and the tangent step of a build of the library, under the argument lists of include/nns.h."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_adjoint_f32.argtypes = [P] * 3 + [I, P, P, P, Z] + [I] * 3 + [D] * 5 + [I, P]
    L.nns_spec_ns_step_tangent_f32.argtypes = [P] * 4 + [I, P, I, P, Z] + [I] * 3 + [D] * 5 + [P, P, ctypes.c_uint64, P, P, I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def check(rc):
        if rc != 0:
            raise RuntimeError('the library refused the call: %d' % rc)

    def adjoint(s, what0, mean, ghat, lam, gbar, work):
        check(L.nns_spec_ns_step_adjoint_f32(p(what0), p(mean), p(ghat), ghat.shape[0], p(lam), p(gbar), p(work), work.numel(), lam.shape[0], s.nx,
                                             s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, what0.shape[0], stream()))

    def tangent(s, what, dwhat, mean, ghat, work, n):
        check(L.nns_spec_ns_step_tangent_f32(p(what), p(dwhat), p(mean), p(ghat), ghat.shape[0], None, 0, p(work), work.numel(), what.shape[0], s.nx,
                                             s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, None, None, 0, None, None, n, stream()))
    return dict(adjoint=adjoint, tangent=tangent)


def timing(args):
    out = []
    parent = direct_calls(args.parent_lib) if args.parent_lib else None
    this = direct_calls(_lib.LIB_PATH)
    steps = args.steps
    for n, B in CASES:
        s = PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG).kolmogorov_forcing(4, 1.0)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        draw = lambda k: dev(O.random_ic(B, n, n, 8, seed=n + B + k, umax=1.0)[0])
        st = s.init(dev(u0), dev(v0))
        s.step(st, 20)                                                    # a developed state
        w, dw, r, r2 = s.vorticity(st), draw(1), draw(2), draw(3)
        g = s.vorticity(s._at_rest(s.ghat.expand(B, -1, -1, -1).contiguous()))
        run = s.second_order_forward(w, dw, steps, forcing=g)
        lam0, dlam0 = s.init_vorticity(r).what, s.init_vorticity(r2).what
        lam, dlam, gbar, dgbar = lam0.clone(), dlam0.clone(), torch.empty_like(lam0), torch.empty_like(lam0)
        work = torch.empty(ops.spec_ns_second_adjoint_workspace(B, n, n), dtype=torch.uint8, device='cuda')
        what, dwhat = run.what0[0].clone(), run.dwhat0[0].clone()

        def restore():
            lam.copy_(lam0)
            dlam.copy_(dlam0)
            what.copy_(run.what0[0])
            dwhat.copy_(run.dwhat0[0])

        second = lambda: ops.spec_ns_second_adjoint_(run.what0, run.dwhat0, run.mean, run.ghat, None, lam, dlam, gbar, dgbar, work, s.ny, s.Lx, s.Ly,
                                                     s.dt, s.nu, s.drag)
        first = lambda calls: (lambda: calls['adjoint'](s, run.what0, run.mean, run.ghat, lam, gbar, work))
        tang = lambda calls: (lambda: calls['tangent'](s, what, dwhat, run.mean, run.ghat, work, steps))
        variants = [('second_adjoint', second), ('adjoint', first(this)), ('tangent_step', tang(this))]
        case = dict(nx=n, ny=n, batch=B)
        restore()
        second()
        bits = (lam.clone(), gbar.clone())
        restore()
        first(this)()
        case['first_order_outputs_bitwise_the_adjoint'] = bool(torch.equal(lam, bits[0]) and torch.equal(gbar, bits[1]))
        if parent:
            for name, make, outs in (('adjoint', first, lambda: (lam.clone(), gbar.clone())), ('tangent_step', tang, lambda: (what.clone(), dwhat.clone()))):
                restore()
                make(this)()
                mine = outs()
                restore()
                make(parent)()
                case[name + '_bitwise_parent_lib'] = bool(all(torch.equal(a, b) for a, b in zip(mine, outs())))
                for tag, calls in (('_parent_lib', parent), ('_direct', this), ('_parent_lib_again', parent)):
                    variants.append((name + tag, make(calls)))

        def product():
            fwd = s.second_order_forward(w, dw, steps, forcing=g)
            return fwd.backward(r, r2)

        def finite_difference():
            for sign in (1.0, -1.0):
                wq = (w + sign * 1e-3 * dw).requires_grad_(True)
                gq = g.clone().requires_grad_(True)
                (s.evolve(wq, steps, forcing=gq) * r).sum().backward()
        variants += [('product', product), ('finite_difference', finite_difference)]
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
        case['second_adjoint_over_adjoint'] = ratio(ts['second_adjoint'], ts['adjoint'])
        case['second_adjoint_over_tangent_step'] = ratio(ts['second_adjoint'], ts['tangent_step'])
        case['product_over_finite_difference'] = ratio(ts['product'], ts['finite_difference'])
        if parent:
            for name in ('adjoint', 'tangent_step'):
                ab = ratio(ts[name + '_direct'], ts[name + '_parent_lib'])
                aa = ratio(ts[name + '_parent_lib_again'], ts[name + '_parent_lib'])
                case[name + '_over_parent_lib'], case[name + '_parent_lib_again_over_parent_lib'] = ab, aa
        case['model_bytes_in_compacted_fields'] = MODEL_C
        case['model_second_adjoint_over_adjoint'] = round(MODEL_C['second_adjoint'] / MODEL_C['adjoint'], 3)
        case['model_second_adjoint_over_tangent_step'] = round(MODEL_C['second_adjoint'] / MODEL_C['tangent_step'], 3)
        case['model_product_over_finite_difference'] = round(MODEL_C['product'] / MODEL_C['finite_difference'], 3)
        out.append(case)
        print(json.dumps(case), flush=True)
        del run, work, lam, dlam, gbar, dgbar, what, dwhat, st
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_second_adjoint_cases as SC
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    rows = []
    for run in SC.RUNS:
        kind, c = run
        d = SC.fields(c)
        f = {k: dev(d[k]) for k in ('w', 'mean', 'g', 'dw', 'r', 'r2')}
        for setting in SC.SETTINGS:
            worst = [0.0, 0.0]
            for dg in (None, 'grid', 'shared'):
                s = SC.solver(kind, c, d['dt'])
                q = SC.dforcing(c, dg)
                fwd = s.second_order_forward(f['w'], f['dw'], SC.NSTEPS, mean=f['mean'], forcing=f['g'], dforcing=None if q is None else dev(q))
                got = fwd.backward(f['r'], f['r2'] if setting == 'generic' else torch.zeros_like(f['r']))
                ref = SC.oracle_second(run, setting, None, dg)
                worst = [max(worst[0], SC.rel(host(got.dwbar), ref[2])), max(worst[1], SC.rel(host(got.dgbar), ref[3]))]
            row = dict(run=SC.run_id(run), setting=setting, steps=SC.NSTEPS, dwbar=float('%.3e' % worst[0]), dgbar=float('%.3e' % worst[1]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return dict(second_adjoint=rows, bound=SC.BOUND, symmetry_measured=SC.SYM_MEASURED, symmetry_bound=SC.SYM_BOUND)


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the new kernels from the amdhsa.kernels block that ends the listing of tools/isa_listing.py."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and any(k in name.group(1) for k in ('PsKeepTangent', 'PsAdjSecond', 'ps_row_adj2_kernel')):
            res[name.group(1)] = dict(vgprs=int(vg.group(1)), scratch_bytes=int(sc.group(1)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=10, help='steps per timing')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's) for the same-process comparison")
    ap.add_argument('--isa-listing', default=None, help='pspec_second_adjoint.s of tools/isa_listing.py (registers and scratch per kernel)')
    ap.add_argument('--no-accuracy', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps, parent_lib=bool(args.parent_lib))
    if not args.no_accuracy:
        rec['accuracy'] = accuracy()
    rec['timing'] = timing(args)
    rec['kernels'] = kernel_resources(args.isa_listing)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_second_adjoint_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
