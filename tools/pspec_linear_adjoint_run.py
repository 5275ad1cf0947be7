"""Measures the reverse mode of the periodic spectral solver's linear step and the complete entry point (nns.periodic.PeriodicSolver.evolve:
nns_spec_ns_step_linear_adjoint_f32 of csrc/pspec_kernels.hip).  Writes ONE JSON record to OUTDIR/pspec_linear_adjoint_run.json and prints it.

    python tools/pspec_linear_adjoint_run.py OUTDIR [--steps 20] [--reps 7] [--commit ID] [--parent-lib PATH] [--name NAME] [--isa-notes FILE] [--no-accuracy]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow and scalar, Kolmogorov force k = 4, drag 0.1; linear: nu_h, p = 4; mu, q = 1; beta of
tools/pspec_linear_run.py; scalar: kappa = nu, G = b = (0, 1)) these take turns within every repetition, each from the same saved state: the
steady-forced and the linear step, the steady-forced and the linear adjoint call, both without and with the buoyant scalar, and forward +
backward through ``advance`` (steady-forced) and ``evolve`` (steady-forced, where it is ``advance``, and linear) with a differentiable forcing.
With --parent-lib also whether the forward steps and the existing adjoints of another build of the library (the parent commit's) loaded into the
same process give the same bits, and the forced step and the flow's adjoint call of this build against the parent's in the same rotation, each
twice (this, parent, parent, this): the ratio of the parent's two turns is the noise the A/B ratio is read against, and this build's second turn
tells a difference between the builds from one between the places in the rotation.  A timing is device events around the work, reported
per step as the median over the repetitions with the spread (max - min) / median; ratios are medians of the per-repetition ratios.

What to compare against: the forward's linear / steady-forced step, 1.016x at 256^2 x 64 and 1.003x at 1024^2 x 8 (profiles/pspec_linear_run.json):
the adjoint moves the same bytes as the steady one plus the table, once per LINEAR launch (6 of the 16), and trades two expm1 for one expm1 and
one sincospi in them.
Accuracy (tests/pspec_linear_adjoint_cases.py, the figures tests/test_gpu_pspec_linear_adjoint.py bounds): wbar, (thetabar,) gbar after 3 steps
against the float64 restatement.  The register and scratch figures of the new kernels come from the code object's metadata (--isa-notes FILE:
the text of `llvm-readelf --notes` on the library, or the amdhsa.kernels block that ends the listing of tools/isa_listing.py)."""
import argparse
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
from pspec_adjoint_run import event_ms, stats, ratio, dev  # noqa: E402
from pspec_linear_run import linear_kw  # noqa: E402
from pspec_scalar_adjoint_run import parent_calls  # noqa: E402

CASES = [(256, 64), (1024, 8)]
DT, NU, DRAG, KAPPA, GRAD, BUOY = 1e-3, 1e-3, 0.1, 1e-3, (0.0, 1.0), (0.0, 1.0)
FORWARD_LINEAR_OVER_FORCED = {256: 1.016, 1024: 1.003}          # profiles/pspec_linear_run.json


def timing(args):
    out = []
    parent = parent_calls(args.parent_lib) if args.parent_lib else None
    for n, B in CASES:
        mk = lambda **kw: PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, **kw).kolmogorov_forcing(4, 1.0)
        sc = dict(kappa=KAPPA, scalar_gradient=GRAD, buoyancy=BUOY)
        forced, linear, forced_sc, linear_sc = mk(), mk(**linear_kw(n)), mk(**sc), mk(**sc, **linear_kw(n))
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 1, umax=1.0)[0]
        st = linear_sc.init(dev(u0), dev(v0), dev(th0))
        linear_sc.step(st, 20)                                            # a developed state
        saved = st.clone()
        sf = PeriodicState(st.what, st.mean, st.work)                     # the same buffers without the scalar
        w0 = forced.vorticity(sf)
        g = forced.vorticity(PeriodicState(forced.ghat, torch.zeros((1, 2), device='cuda'), torch.empty(0, dtype=torch.uint8, device='cuda')))
        rw, rt = (dev(f) for f in O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0))
        steps = args.steps
        what0 = torch.empty((steps,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        that0 = torch.empty_like(what0)
        lam0 = forced.init_vorticity(rw).what
        mu0 = forced_sc.init(torch.zeros_like(rt), torch.zeros_like(rt), rt).that
        lam, mu, gbar = lam0.clone(), mu0.clone(), torch.empty_like(lam0)
        awork = torch.empty(ops.spec_ns_scalar_adjoint_workspace(B, n, n), dtype=torch.uint8, device='cuda')
        lin = linear._linear_of(st)

        def restore():
            st.what.copy_(saved.what)
            st.that.copy_(saved.that)

        def keep():
            for k in range(steps):
                what0[k].copy_(st.what)
                that0[k].copy_(st.that)
                linear_sc.step(st, 1)

        def adjoint(s, scalar, table):
            lam.copy_(lam0)
            mu.copy_(mu0)
            box = (n, s.Lx, s.Ly, s.dt)
            if table is not None:
                ops.spec_ns_step_linear_adjoint_(what0, that0 if scalar else None, st.mean, s.ghat, lam, mu if scalar else None, gbar, awork, *box,
                                                 KAPPA, GRAD, BUOY, table)
            elif scalar:
                ops.spec_ns_step_scalar_adjoint_(what0, that0, st.mean, s.ghat, lam, mu, gbar, awork, *box, s.nu, s.drag, KAPPA, GRAD, BUOY)
            else:
                ops.spec_ns_step_adjoint_(what0, st.mean, s.ghat, lam, gbar, awork, *box, s.nu, s.drag)

        def autograd(call):
            a, f = (x.detach().requires_grad_(True) for x in (w0, g))
            (call(a, steps, mean=st.mean, forcing=f) * rw).sum().backward()

        variants = [('forced_step', lambda: forced.step(sf, steps)), ('linear_step', lambda: linear.step(sf, steps)),
                    ('forced_scalar_step', lambda: forced_sc.step(st, steps)), ('linear_scalar_step', lambda: linear_sc.step(st, steps)),
                    ('forced_adjoint_call', lambda: adjoint(forced, False, None)), ('linear_adjoint_call', lambda: adjoint(linear, False, lin)),
                    ('forced_scalar_adjoint_call', lambda: adjoint(forced_sc, True, None)),
                    ('linear_scalar_adjoint_call', lambda: adjoint(linear_sc, True, lin)),
                    ('forced_advance_forward_backward', lambda: autograd(forced.advance)),
                    ('forced_evolve_forward_backward', lambda: autograd(forced.evolve)),
                    ('linear_evolve_forward_backward', lambda: autograd(linear.evolve))]
        case = dict(nx=n, ny=n, batch=B, kept_bytes_per_step=int(8 * B * forced.my1 * n))
        restore()
        keep()                                                            # what0, that0 for the adjoint calls
        if parent:
            for name, s in (('forced', forced), ('buoyant', forced_sc)):
                restore()
                s.step(sf if name == 'forced' else st, 3)
                mine = (st.what.clone(), st.that.clone())
                restore()
                parent[name](s, st, 3)
                case[name + '_step_bitwise_parent_lib'] = bool(torch.equal(mine[0], st.what) and torch.equal(mine[1], st.that))
            adjoint(forced, False, None)
            mine = (lam.clone(), gbar.clone())
            lam.copy_(lam0)
            parent['adjoint'](forced, what0, st.mean, lam, gbar, awork)
            case['flow_adjoint_bitwise_parent_lib'] = bool(torch.equal(mine[0], lam) and torch.equal(mine[1], gbar))
            adjoint(forced_sc, True, None)
            mine = (lam.clone(), mu.clone(), gbar.clone())
            lam.copy_(lam0)
            mu.copy_(mu0)
            parent['scalar_adjoint'](forced_sc, what0, that0, st.mean, lam, mu, gbar, awork)
            case['scalar_adjoint_bitwise_parent_lib'] = bool(all(torch.equal(a, b) for a, b in zip(mine, (lam, mu, gbar))))
            # this build and the parent's under the same direct calls, each twice (this, parent, parent, this): the A/A ratios are the noise,
            # and this build's second turn shows what the place in the rotation does to the first
            this = parent_calls(_lib.LIB_PATH)
            for tag, calls in (('', this), ('_parent_lib', parent), ('_parent_lib_again', parent), ('_again', this)):
                def direct_adjoint(calls=calls):
                    lam.copy_(lam0)
                    calls['adjoint'](forced, what0, st.mean, lam, gbar, awork)
                variants.append(('flow_adjoint_direct' + tag, direct_adjoint))
                variants.append(('forced_step_direct' + tag, lambda calls=calls: calls['forced'](forced, st, steps)))
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
        r = lambda a, b: ratio(ts[a], ts[b])
        case['linear_over_forced_step'] = r('linear_step', 'forced_step')
        case['linear_over_forced_scalar_step'] = r('linear_scalar_step', 'forced_scalar_step')
        case['linear_over_forced_adjoint'] = r('linear_adjoint_call', 'forced_adjoint_call')
        case['linear_over_forced_scalar_adjoint'] = r('linear_scalar_adjoint_call', 'forced_scalar_adjoint_call')
        case['linear_adjoint_over_linear_step'] = r('linear_adjoint_call', 'linear_step')
        case['linear_scalar_adjoint_over_linear_scalar_step'] = r('linear_scalar_adjoint_call', 'linear_scalar_step')
        case['forced_evolve_over_advance'] = r('forced_evolve_forward_backward', 'forced_advance_forward_backward')
        case['linear_evolve_over_advance'] = r('linear_evolve_forward_backward', 'forced_advance_forward_backward')
        case['expected_linear_over_forced'] = FORWARD_LINEAR_OVER_FORCED[n]
        if parent:
            for what in ('flow_adjoint_direct', 'forced_step_direct'):
                ab, aa = r(what, what + '_parent_lib'), r(what + '_parent_lib_again', what + '_parent_lib')
                case[what + '_over_parent_lib'], case[what + '_parent_lib_again_over_parent_lib'] = ab, aa
                case[what + '_median_inside_parent_lib_noise'] = bool(aa['min'] <= ab['median'] <= aa['max'])
                case[what + '_again_over_parent_lib'] = r(what + '_again', what + '_parent_lib')
                case[what + '_again_over_first_turn'] = r(what + '_again', what)
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, sf, saved, what0, that0, awork
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_linear_adjoint_cases as LA
    cplx = lambda t: t.cpu().numpy().astype(np.float64)[..., 0] + 1j * t.cpu().numpy().astype(np.float64)[..., 1]
    rows = []
    for kind, c in LA.RUNS:
        nx, ny, B, Lx, Ly, _ = c
        d = LA.inputs(c)
        s = LA.solver(kind, c, d['dt'])
        scalar = kind in ('scalar', 'buoyant')
        ghat = s.init(dev(d['fx']), dev(d['fy'])).what
        st = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']) if scalar else None)
        what0 = torch.empty((LA.NSTEPS,) + tuple(st.what.shape), dtype=torch.float32, device='cuda')
        that0 = torch.empty_like(what0) if scalar else None
        s.ghat = ghat
        for k in range(LA.NSTEPS):
            what0[k].copy_(st.what)
            if scalar:
                that0[k].copy_(st.that)
            s.step(st, 1)
        lam = s.init_vorticity(dev(d['rw'])).what
        z = torch.zeros((B, nx, ny), device='cuda')
        mu = s.init(z, z, dev(d['rt'])).that if scalar else None
        gbar = torch.empty_like(lam)
        size = ops.spec_ns_scalar_adjoint_workspace if scalar else ops.spec_ns_adjoint_workspace
        work = torch.empty(size(B, nx, ny), dtype=torch.uint8, device='cuda')
        ops.spec_ns_step_linear_adjoint_(what0, that0, st.mean, ghat, lam, mu, gbar, work, ny, Lx, Ly, s.dt, s.kappa if scalar else 0.0,
                                         s.scalar_gradient, s.buoyancy, s._linear_of(st))
        got = (lam, mu, gbar) if scalar else (lam, gbar)
        errs = [float('%.3e' % LA.rel(cplx(g), r)) for g, r in zip(got, LA.oracle_gradient(kind, c))]
        row = dict(run=LA.run_id((kind, c)), steps=LA.NSTEPS, bound=LA.bound(kind), **dict(zip(('wbar', 'thetabar', 'gbar') if scalar else ('wbar', 'gbar'), errs)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(gradients=rows, bound_flow=LA.BOUND_FLOW, bound_scalar=LA.BOUND_SCALAR)


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the linear adjoint and the linear stage-keeping kernels from the text of `llvm-readelf --notes`."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and (re.search(r'PsAdj(Scalar)?Linear', name.group(1)) or ('PsLinear' in name.group(1) and 'PsKeep' in name.group(1))):
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
    ap.add_argument('--name', default='pspec_linear_adjoint_run', help='the record is OUTDIR/NAME.json')
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
