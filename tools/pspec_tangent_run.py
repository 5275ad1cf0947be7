"""Measures the forward mode of the periodic spectral solver's step (nns.periodic.PeriodicSolver.step_tangent: nns_spec_ns_step_tangent_f32 of
csrc/pspec_kernels.hip).  Writes ONE JSON record to OUTDIR/pspec_tangent_run.json and prints it.

    python tools/pspec_tangent_run.py OUTDIR [--steps 20] [--reps 7] [--commit ID] [--parent-lib PATH] [--name NAME] [--isa-notes FILE] [--no-accuracy]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow, scalar and perturbation, Kolmogorov force k = 4, drag 0.1, kappa = nu, G = (0, 1)) these
take turns within every repetition, each from the same saved state: the flow-only forced step, the passive-scalar step, the tangent step and,
with --parent-lib, the forced and the scalar step of this build and of another build of the library (the parent commit's) under the same
direct call, the parent's twice with this build's turn between them (so each of the three follows a step of its own footprint, not the tangent
step's larger one): the ratio of the parent's two turns is the noise the A/B ratio is read against; also whether both builds give the same bits.  A timing is device events around the work, reported per step as the median over the repetitions with the spread
(max - min) / median; ratios are medians of the per-repetition ratios.

The byte model to compare against, in compacted fields c moved per step: the flow's step 50c, the scalar's 84c, the
tangent's 100c -- 12 fields in its workspace against 6 -- so 2.0x the flow step and 1.19x the scalar step.
Accuracy (tests/pspec_tangent_cases.py, the figures tests/test_gpu_pspec_tangent.py bounds): the tangent spectrum after 3 steps against the
float64 restatement, without and with a source perturbation, and the dot-product identity against the backward of ``evolve``.  The register
and scratch figures of the new kernels come from the code object's metadata (--isa-notes FILE: the text of `llvm-readelf --notes` on the
library, or the amdhsa.kernels block that ends the listing of tools/isa_listing.py, made at build time)."""
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
from nns import _lib  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402
from pspec_adjoint_run import event_ms, stats, ratio, dev  # noqa: E402

CASES = [(256, 64), (1024, 8)]
DT, NU, DRAG, KAPPA, GRAD = 1e-3, 1e-3, 0.1, 1e-3, (0.0, 1.0)
MODEL_C = dict(flow_step=50, scalar_step=84, tangent_step=100)


def direct_calls(path):
    """The forced and the scalar step of a build of the library, under the argument lists of include/nns.h."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_forced_f32.argtypes = [P] * 3 + [I, P, Z] + [I] * 3 + [D] * 5 + [I, P]
    L.nns_spec_ns_step_scalar_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 8 + [I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def check(rc):
        if rc != 0:
            raise RuntimeError('the library refused the call: %d' % rc)

    def forced(s, st, n):
        check(L.nns_spec_ns_step_forced_f32(p(st.what), p(st.mean), p(s.ghat), 1, p(st.work), st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly,
                                            s.dt, s.nu, s.drag, n, stream()))

    def scalar(s, st, n):
        check(L.nns_spec_ns_step_scalar_f32(p(st.what), p(st.that), p(st.mean), p(s.ghat), 1, p(st.work), st.work.numel(), st.batch, s.nx, s.ny,
                                            s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient[0], s.scalar_gradient[1], n, stream()))
    return dict(forced=forced, scalar=scalar)


def timing(args):
    out = []
    parent = direct_calls(args.parent_lib) if args.parent_lib else None
    this = direct_calls(_lib.LIB_PATH) if parent else None
    for n, B in CASES:
        mk = lambda **kw: PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, **kw).kolmogorov_forcing(4, 1.0)
        flow, sca = mk(), mk(kappa=KAPPA, scalar_gradient=GRAD)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 1, umax=1.0)[0]
        dw0 = O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0)[0]
        st = sca.init(dev(u0), dev(v0), dev(th0))
        sca.step(st, 20)                                                  # a developed state
        saved = st.clone()
        fl = flow.init(dev(u0), dev(v0))                                  # the flow's state: the same spectrum, no scalar
        dwhat0 = flow.init_vorticity(dev(dw0)).what
        dwhat = dwhat0.clone()
        steps = args.steps

        def restore():
            st.what.copy_(saved.what)
            st.that.copy_(saved.that)
            fl.what.copy_(saved.what)
            dwhat.copy_(dwhat0)

        variants = [('flow_step', lambda: flow.step(fl, steps)), ('scalar_step', lambda: sca.step(st, steps)),
                    ('tangent_step', lambda: flow.step_tangent(fl, dwhat, steps))]
        case = dict(nx=n, ny=n, batch=B)
        if parent:
            for name, s, state in (('forced', flow, fl), ('scalar', sca, st)):
                restore()
                this[name](s, state, 3)
                mine = (st.what.clone(), st.that.clone(), fl.what.clone())
                restore()
                parent[name](s, state, 3)
                case[name + '_step_bitwise_parent_lib'] = bool(all(torch.equal(a, b) for a, b in zip(mine, (st.what, st.that, fl.what))))
            for name, s, state in (('forced', flow, fl), ('scalar', sca, st)):
                for tag, calls in (('_parent_lib', parent), ('', this), ('_parent_lib_again', parent)):       # this build's turn between the parent's two
                    variants.append((name + '_step_direct' + tag, lambda calls=calls, name=name, s=s, state=state: calls[name](s, state, steps)))
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
        case['tangent_over_flow_step'] = ratio(ts['tangent_step'], ts['flow_step'])
        case['tangent_over_scalar_step'] = ratio(ts['tangent_step'], ts['scalar_step'])
        if parent:
            for name in ('forced', 'scalar'):
                ab = ratio(ts[name + '_step_direct'], ts[name + '_step_direct_parent_lib'])
                aa = ratio(ts[name + '_step_direct_parent_lib_again'], ts[name + '_step_direct_parent_lib'])
                case[name + '_step_over_parent_lib'], case[name + '_parent_lib_again_over_parent_lib'] = ab, aa
                case[name + '_step_median_inside_parent_lib_noise'] = bool(aa['min'] <= ab['median'] <= aa['max'])
        case['model_bytes_in_compacted_fields'] = MODEL_C
        case['model_tangent_over_flow_step'] = round(MODEL_C['tangent_step'] / MODEL_C['flow_step'], 3)
        case['model_tangent_over_scalar_step'] = round(MODEL_C['tangent_step'] / MODEL_C['scalar_step'], 3)
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, saved, fl, dwhat, dwhat0
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_tangent_cases as TC
    cplx = lambda t: t.cpu().numpy().astype(np.float64)[..., 0] + 1j * t.cpu().numpy().astype(np.float64)[..., 1]
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    rows, dots = [], []
    for run in TC.RUNS:
        kind, c = run
        d = TC.inputs(c)
        errs = []
        for dg in (None, 'grid', 'shared'):
            s = TC.solver(kind, c, d['dt'])
            s.set_forcing(dev(d['fx']), dev(d['fy']))
            state = s.init(dev(d['u0']), dev(d['v0']))
            dwhat = s.init_vorticity(dev(d['dw'])).what
            dwhat[:, 0, 0, 0] = TC.DW_00 * c[0] * c[1]
            g = TC.source(c, dg)
            s.step_tangent(state, dwhat, TC.NSTEPS, dforcing=None if g is None else dev(g))
            errs.append(float('%.3e' % TC.rel(cplx(dwhat), TC.oracle_tangent(run, None, dg))))
        row = dict(run=TC.run_id(run), steps=TC.NSTEPS, no_source=errs[0], source_per_grid=errs[1], source_shared=errs[2])
        rows.append(row)
        print(json.dumps(row), flush=True)
    c = TC.CASES[0]
    d = TC.inputs(c)
    for kind in TC.KINDS:
        s = TC.solver(kind, c, d['dt'])
        st = s.init(dev(d['u0']), dev(d['v0']))
        w, mean = s.vorticity(st).requires_grad_(True), st.mean.clone()
        g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
        dw, dg = s.vorticity(s.init_vorticity(dev(d['dw']))), s.vorticity(s.init_vorticity(dev(d['dforcing'])))
        r = dev(d['r'])
        kw = dict(mean=mean, clock=5, noise_ids=[2, 0, 7])
        (s.evolve(w, TC.NSTEPS, forcing=g, **kw) * r).sum().backward()
        dw_out = s.evolve_tangent(w.detach(), dw, TC.NSTEPS, forcing=g.detach(), dforcing=dg, **kw)[1]
        lhs = float((host(dw_out) * host(r)).sum())
        rhs = float((host(w.grad) * host(dw)).sum() + (host(g.grad) * host(dg)).sum())
        row = dict(kind=kind, case=TC.run_id((kind, c)), scaled_difference=float('%.3e' % (abs(lhs - rhs) / (np.linalg.norm(host(dw_out)) * np.linalg.norm(host(r))))))
        dots.append(row)
        print(json.dumps(row), flush=True)
    return dict(tangents=rows, bound=TC.BOUND, dot_product=dots, dot_bound=TC.DOT_BOUND)


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the tangent kernels from the text of `llvm-readelf --notes` on the library."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and any(k in name.group(1) for k in ('PsTangent', 'ps_row_tan_kernel')):
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
    ap.add_argument('--name', default='pspec_tangent_run', help='the record is OUTDIR/NAME.json')
    ap.add_argument('--no-accuracy', action='store_true')
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
