"""Measures the forward mode of the periodic spectral solver's step with a scalar (nns.periodic.PeriodicSolver.step_tangent_scalar:
nns_spec_ns_step_scalar_tangent_f32 of csrc/pspec_kernels.hip).  Writes ONE JSON record to OUTDIR/pspec_scalar_tangent_run.json and prints it.

    python tools/pspec_scalar_tangent_run.py OUTDIR [--steps 20] [--reps 7] [--commit ID] [--parent-lib PATH] [--name NAME] [--isa-notes FILE] [--no-accuracy]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow, scalar and perturbations, Kolmogorov force k = 4, drag 0.1, kappa = nu, G = (0, 1),
b = (0, 1) for the buoyant forms) these take turns within every repetition, each from the same saved state: the passive-scalar step, the
buoyant step, the flow's tangent step, the passive and the buoyant scalar-tangent step and, with --parent-lib, the scalar, the buoyant and
the flow-tangent step of this build and of another build of the library (the parent commit's) under the same direct call, the parent's twice
with this build's turn between them: the ratio of the parent's two turns is the noise the A/B ratio is read against; also whether both
builds give the same bits.  A timing is device events around the work, reported per step as the median over the repetitions with the spread
(max - min) / median; ratios are medians of the per-repetition ratios.

The byte model to compare against, in compacted fields c moved per step: a step with g fields of G, p of Ph and s
spectra moves 4 x 2 (g + p) + 10 s -- the scalar step 4 x 2 x 8 + 20 = 84c, the flow's tangent 4 x 2 x 10 + 20 = 100c, the scalar tangent
(20 fields in its workspace: g = 12, p = 4, s = 4) 4 x 2 x 16 + 40 = 168c: 2.0x the scalar step, which is also what the finite-difference
alternative costs (two scalar steps for a one-sided difference, with its truncation and cancellation errors).  The second read of G fields
6 and 7 by the row pass (its seventh inverse transform) is not in the model: 8c more per step if it missed every cache.
Accuracy (tests/pspec_scalar_tangent_cases.py, the figures tests/test_gpu_pspec_scalar_tangent.py bounds): (dw^, dtheta^) after 3 steps
against the float64 restatement, without and with a source perturbation, and the dot-product identity against the backward of ``evolve``.
The register and scratch figures of the new kernels come from the code object's metadata (--isa-notes FILE: the text of `llvm-readelf
--notes` on the library, or the amdhsa.kernels block that ends the listing of tools/isa_listing.py, made at build time)."""
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
DT, NU, DRAG, KAPPA, GRAD, BUOY = 1e-3, 1e-3, 0.1, 1e-3, (0.0, 1.0), (0.0, 1.0)
MODEL_C = dict(scalar_step=84, tangent_step=100, scalar_tangent_step=168, two_scalar_steps=168)


def direct_calls(path):
    """The scalar, the buoyant and the flow-tangent step of a build of the library, under the argument lists of include/nns.h."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_scalar_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 8 + [I, P]
    L.nns_spec_ns_step_buoyant_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 10 + [I, P]
    L.nns_spec_ns_step_tangent_f32.argtypes = [P] * 4 + [I, P, I, P, Z] + [I] * 3 + [D] * 5 + [P, P, ctypes.c_uint64, P, P, I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def check(rc):
        if rc != 0:
            raise RuntimeError('the library refused the call: %d' % rc)

    def scalar(s, st, dwhat, n):
        check(L.nns_spec_ns_step_scalar_f32(p(st.what), p(st.that), p(st.mean), p(s.ghat), 1, p(st.work), st.work.numel(), st.batch, s.nx, s.ny,
                                            s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient[0], s.scalar_gradient[1], n, stream()))

    def buoyant(s, st, dwhat, n):
        check(L.nns_spec_ns_step_buoyant_f32(p(st.what), p(st.that), p(st.mean), p(s.ghat), 1, p(st.work), st.work.numel(), st.batch, s.nx, s.ny,
                                             s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient[0], s.scalar_gradient[1], s.buoyancy[0],
                                             s.buoyancy[1], n, stream()))

    def tangent(s, st, dwhat, n):
        check(L.nns_spec_ns_step_tangent_f32(p(st.what), p(dwhat), p(st.mean), p(s.ghat), 1, None, 0, p(st.work), st.work.numel(), st.batch, s.nx,
                                             s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, None, None, 0, None, None, n, stream()))
    return dict(scalar=scalar, buoyant=buoyant, tangent=tangent)


def timing(args):
    out = []
    parent = direct_calls(args.parent_lib) if args.parent_lib else None
    this = direct_calls(_lib.LIB_PATH) if parent else None
    for n, B in CASES:
        mk = lambda **kw: PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, **kw).kolmogorov_forcing(4, 1.0)
        flow, sca, buo = mk(), mk(kappa=KAPPA, scalar_gradient=GRAD), mk(kappa=KAPPA, scalar_gradient=GRAD, buoyancy=BUOY)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0, dw0, dth0 = (O.random_ic(B, n, n, 8, seed=n + B + k, umax=1.0)[0] for k in (1, 2, 3))
        st = sca.init(dev(u0), dev(v0), dev(th0))
        sca.step(st, 20)                                                  # a developed state
        st.work = sca._work(ops.spec_ns_scalar_tangent_workspace, B, st.what.device, have=st.work)      # one workspace serves every variant
        saved = st.clone()
        fl = flow.init(dev(u0), dev(v0))                                  # the flow's state: the same spectrum, no scalar
        fl.work = st.work
        dwhat0 = flow.init_vorticity(dev(dw0)).what
        dthat0 = sca.init(dev(u0), dev(v0), dev(dth0)).that
        dwhat, dthat = dwhat0.clone(), dthat0.clone()
        steps = args.steps

        def restore():
            st.what.copy_(saved.what)
            st.that.copy_(saved.that)
            fl.what.copy_(saved.what)
            dwhat.copy_(dwhat0)
            dthat.copy_(dthat0)

        variants = [('scalar_step', lambda: sca.step(st, steps)), ('buoyant_step', lambda: buo.step(st, steps)),
                    ('tangent_step', lambda: flow.step_tangent(fl, dwhat, steps)),
                    ('scalar_tangent_step', lambda: sca.step_tangent_scalar(st, dwhat, dthat, steps)),
                    ('buoyant_tangent_step', lambda: buo.step_tangent_scalar(st, dwhat, dthat, steps))]
        case = dict(nx=n, ny=n, batch=B)
        triples = (('scalar', sca, st), ('buoyant', buo, st), ('tangent', flow, fl))
        if parent:
            for name, s, state in triples:
                restore()
                this[name](s, state, dwhat, 3)
                mine = (st.what.clone(), st.that.clone(), fl.what.clone(), dwhat.clone())
                restore()
                parent[name](s, state, dwhat, 3)
                case[name + '_step_bitwise_parent_lib'] = bool(all(torch.equal(a, b) for a, b in zip(mine, (st.what, st.that, fl.what, dwhat))))
            for name, s, state in triples:
                for tag, calls in (('_parent_lib', parent), ('', this), ('_parent_lib_again', parent)):       # this build's turn between the parent's two
                    variants.append((name + '_step_direct' + tag, lambda calls=calls, name=name, s=s, state=state: calls[name](s, state, dwhat, steps)))
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
        case['scalar_tangent_over_scalar_step'] = ratio(ts['scalar_tangent_step'], ts['scalar_step'])
        case['buoyant_tangent_over_buoyant_step'] = ratio(ts['buoyant_tangent_step'], ts['buoyant_step'])
        case['scalar_tangent_over_tangent_step'] = ratio(ts['scalar_tangent_step'], ts['tangent_step'])
        if parent:
            for name, _, _ in triples:
                ab = ratio(ts[name + '_step_direct'], ts[name + '_step_direct_parent_lib'])
                aa = ratio(ts[name + '_step_direct_parent_lib_again'], ts[name + '_step_direct_parent_lib'])
                case[name + '_step_over_parent_lib'], case[name + '_parent_lib_again_over_parent_lib'] = ab, aa
                case[name + '_step_median_inside_parent_lib_noise'] = bool(aa['min'] <= ab['median'] <= aa['max'])
        case['model_bytes_in_compacted_fields'] = MODEL_C
        case['model_scalar_tangent_over_scalar_step'] = round(MODEL_C['scalar_tangent_step'] / MODEL_C['scalar_step'], 3)
        case['model_scalar_tangent_over_tangent_step'] = round(MODEL_C['scalar_tangent_step'] / MODEL_C['tangent_step'], 3)
        case['finite_difference_over_scalar_step'] = 2.0
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, saved, fl, dwhat, dwhat0, dthat, dthat0
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_scalar_tangent_cases as TC
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    cplx = lambda t: host(t)[..., 0] + 1j * host(t)[..., 1]
    fig = lambda x: float('%.3e' % x)
    rows, dots = [], []
    for run in TC.RUNS:
        kind, c = run
        d = TC.inputs(c)
        errs = []
        for dg in (None, 'grid', 'shared'):
            s = TC.solver(kind, c, d['dt'])
            s.set_forcing(dev(d['fx']), dev(d['fy']))
            state = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']))
            dwhat = s.init_vorticity(dev(d['dw'])).what
            dwhat[:, 0, 0, 0] = TC.DW_00 * c[0] * c[1]
            dthat = s.init(dev(d['u0']), dev(d['v0']), dev(d['dtheta'])).that
            g = TC.source(c, dg)
            s.step_tangent_scalar(state, dwhat, dthat, TC.steps(run), dforcing=None if g is None else dev(g))
            ref = TC.oracle_tangent(run, None, dg)
            errs.append((fig(TC.rel(cplx(dwhat), ref[0])), fig(TC.rel(cplx(dthat), ref[1]))))
        row = dict(run=TC.run_id(run), steps=TC.steps(run), dw=dict(no_source=errs[0][0], source_per_grid=errs[1][0], source_shared=errs[2][0]),
                   dtheta=dict(no_source=errs[0][1], source_per_grid=errs[1][1], source_shared=errs[2][1]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    c = TC.CASES[0]
    d = TC.inputs(c)
    for kind in TC.DOT_KINDS:
        s = TC.solver(kind, c, d['dt'])
        st = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']))
        w, theta, mean = s.vorticity(st).requires_grad_(True), s.scalar(st).requires_grad_(True), st.mean.clone()
        g = s.vorticity(s.init(dev(d['fx']), dev(d['fy']))).requires_grad_(True)
        dw, dg = s.vorticity(s.init_vorticity(dev(d['dw']))), s.vorticity(s.init_vorticity(dev(d['dforcing'])))
        dth = s.scalar(s.init(dev(d['u0']), dev(d['v0']), dev(d['dtheta'])))
        rw, rt = dev(d['rw']), dev(d['rt'])
        kw = dict(mean=mean, clock=5, noise_ids=[2, 0, 7])
        ow, ot = s.evolve(w, TC.NSTEPS, theta=theta, forcing=g, **kw)
        ((ow * rw).sum() + (ot * rt).sum()).backward()
        jw, jt = s.evolve_tangent_scalar(w.detach(), theta.detach(), dw, dth, TC.NSTEPS, forcing=g.detach(), dforcing=dg, **kw)[2:]
        dot = lambda a, b: float((host(a) * host(b)).sum())
        norm = lambda *a: float(np.sqrt(sum(np.linalg.norm(host(x)) ** 2 for x in a)))
        lhs, rhs = dot(jw, rw) + dot(jt, rt), dot(w.grad, dw) + dot(theta.grad, dth) + dot(g.grad, dg)
        row = dict(kind=kind, case=TC.run_id((kind, c)), scaled_difference=fig(abs(lhs - rhs) / (norm(jw, jt) * norm(rw, rt))))
        dots.append(row)
        print(json.dumps(row), flush=True)
    return dict(tangents=rows, bound_dw=TC.BOUND_W, bound_dtheta=TC.BOUND_T, dot_product=dots, dot_bound=TC.DOT_BOUND)


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the scalar tangent's kernels from the text of `llvm-readelf --notes` on the library."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and any(k in name.group(1) for k in ('PsTangentScalar', 'ps_row_tan_scalar_kernel')):
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
    ap.add_argument('--name', default='pspec_scalar_tangent_run', help='the record is OUTDIR/NAME.json')
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
