"""Measures K tangent pairs on one base with a scalar of the periodic spectral solver (nns.periodic.PeriodicSolver.step_tangents_scalar:
nns_spec_ns_step_scalar_tangents_f32 of csrc/pspec_scalar_tangents.hip) against K calls of the single pair's step
(nns_spec_ns_step_scalar_tangent_f32), the cost of one orthonormalisation, and the existing steps against another build of the library.
Writes ONE JSON record to OUTDIR/pspec_scalar_tangents_run.json and prints it.

    python tools/pspec_scalar_tangents_run.py OUTDIR [--steps 10] [--reps 7] [--commit ID] [--parent-lib PATH] [--name NAME] [--isa-listing FILE]

Timing: at 256^2 with B K = 64 and 1024^2 with B K = 8, for K = 2, 4, 8, passive (b = 0) and buoyant (|m| <= 8 flow, scalar and perturbations,
Kolmogorov force k = 4, drag 0.1), these take turns within every repetition, each from the same saved state: one step_tangents_scalar call
with K pairs on B grids; K calls of nns_spec_ns_step_scalar_tangent_f32 on K clones of the state, one member each -- with --parent-lib through
another build of the library (the parent commit's) loaded into the same process, else through this build, under the same direct call -- and
that sequence once more, so that the ratio of its two turns is the noise the shared / separate ratio is read against.  Also whether the shared
call's members and base are the bits of the separate calls.  A timing is device events around the work, reported per step as the median over
the repetitions with the spread (max - min) / median; ratios are medians of the per-repetition ratios.  One orthonormalize_tangents_scalar is
timed in the same turns and given in units of one shared step.

With --parent-lib also, at both shapes: the scalar, the buoyant, the flow-tangent, the K = 4 tangents and the scalar-tangent step of this
build and of the parent's under the same direct call, the parent's twice with this build's turn between them (bitwise equal or not, and
the A/B ratio beside the A/A ratio).

The byte model to compare against, in compacted fields c moved per step: the scalar step moves 84c and every pair 84c
more, but the base's share is moved once per call: (84 + 84 K) c shared against 168 K c separate, (1 + K) / (2 K).
The register, LDS and scratch figures of the new kernels come from the listing of tools/isa_listing.py (--isa-listing: pspec_scalar_tangents.s)."""
import argparse
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pspec_oracle as O  # noqa: E402
from nns import _lib, ops  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402
from pspec_adjoint_run import event_ms, stats, ratio, dev  # noqa: E402

CASES = [(256, 64), (1024, 8)]            # (n, B K)
KS = (2, 4, 8)
DT, NU, DRAG, KAPPA, GRAD, BUOY = 1e-3, 1e-3, 0.1, 1e-3, (0.0, 1.0), (0.0, 1.0)
I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t


def direct_calls(path):
    """The existing steps of a build of the library, under the argument lists of include/nns.h: name -> call(s, st, dwhat, dthat, n)."""
    L = ctypes.CDLL(path)
    L.nns_spec_ns_step_scalar_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 8 + [I, P]
    L.nns_spec_ns_step_buoyant_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 10 + [I, P]
    L.nns_spec_ns_step_tangent_f32.argtypes = [P] * 4 + [I, P, I, P, Z] + [I] * 3 + [D] * 5 + [P, P, ctypes.c_uint64, P, P, I, P]
    L.nns_spec_ns_step_tangents_f32.argtypes = [P, P, I, P, P, I, P, Z] + [I] * 3 + [D] * 5 + [P, P, ctypes.c_uint64, P, P, I, P]
    L.nns_spec_ns_step_scalar_tangent_f32.argtypes = [P] * 6 + [I, P, I, P, Z] + [I] * 3 + [D] * 10 + [P, P, ctypes.c_uint64, P, P, I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def check(rc):
        if rc != 0:
            raise RuntimeError('the library refused the call: %d' % rc)
    box = lambda s, st: (p(st.work), st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag)

    def scalar(s, st, dwhat, dthat, n):
        check(L.nns_spec_ns_step_scalar_f32(p(st.what), p(st.that), p(st.mean), p(s.ghat), 1, *box(s, st), s.kappa, *s.scalar_gradient, n, stream()))

    def buoyant(s, st, dwhat, dthat, n):
        check(L.nns_spec_ns_step_buoyant_f32(p(st.what), p(st.that), p(st.mean), p(s.ghat), 1, *box(s, st), s.kappa, *s.scalar_gradient, *s.buoyancy,
                                             n, stream()))

    def tangent(s, st, dwhat, dthat, n):
        check(L.nns_spec_ns_step_tangent_f32(p(st.what), p(dwhat[0]), p(st.mean), p(s.ghat), 1, None, 0, *box(s, st), None, None, 0, None, None, n,
                                             stream()))

    def tangents(s, st, dwhat, dthat, n):
        check(L.nns_spec_ns_step_tangents_f32(p(st.what), p(dwhat), dwhat.shape[0], p(st.mean), p(s.ghat), 1, *box(s, st), None, None, 0, None, None, n,
                                              stream()))

    def scalar_tangent(s, st, dwhat, dthat, n, k=0):
        check(L.nns_spec_ns_step_scalar_tangent_f32(p(st.what), p(st.that), p(dwhat[k]), p(dthat[k]), p(st.mean), p(s.ghat), 1, None, 0, *box(s, st),
                                                    s.kappa, *s.scalar_gradient, *s.buoyancy, None, None, 0, None, None, n, stream()))
    return dict(scalar=scalar, buoyant=buoyant, tangent=tangent, tangents=tangents, scalar_tangent=scalar_tangent)


def fields(n, B, K):
    u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
    th0 = O.random_ic(B, n, n, 8, seed=n + B + 1, umax=1.0)[0]
    dw = torch.stack([dev(O.random_ic(B, n, n, 8, seed=n + B + 2 + 2 * k, umax=1.0)[0]) for k in range(K)])
    dth = torch.stack([dev(O.random_ic(B, n, n, 8, seed=n + B + 3 + 2 * k, umax=1.0)[0]) for k in range(K)])
    return dev(u0), dev(v0), dev(th0), dw, dth


def shared_against_separate(args, single):
    out = []
    for n, BK in CASES:
        for K in KS:
            for kind, b in (('passive', (0.0, 0.0)), ('buoyant', BUOY)):
                B = BK // K
                s = PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, kappa=KAPPA, scalar_gradient=GRAD, buoyancy=b).kolmogorov_forcing(4, 1.0)
                u0, v0, th0, dw, dth = fields(n, B, K)
                st = s.init(u0, v0, th0)
                s.step(st, 20)                                            # a developed state
                saved = st.clone()
                w0, t0 = s.init_tangents_scalar(dw, dth)
                s.orthonormalize_tangents_scalar(w0, t0)
                dwhat, dthat = w0.clone(), t0.clone()
                s.step_tangents_scalar(st, dwhat, dthat, 1)               # grows the workspace
                clones = [st.clone() for _ in range(K)]
                for c in clones:
                    c.work = torch.empty(ops.spec_ns_scalar_tangent_workspace(B, n, n), dtype=torch.uint8, device='cuda')
                steps = args.steps

                def restore():
                    for c in clones + [st]:
                        c.what.copy_(saved.what)
                        c.that.copy_(saved.that)
                    dwhat.copy_(w0)
                    dthat.copy_(t0)

                def separate(nsteps=steps):
                    for k, c in enumerate(clones):
                        single(s, c, dwhat, dthat, nsteps, k)
                variants = [('separate', separate), ('shared', lambda: s.step_tangents_scalar(st, dwhat, dthat, steps)), ('separate_again', separate),
                            ('orthonormalize', lambda: s.orthonormalize_tangents_scalar(dwhat, dthat))]
                case = dict(nx=n, ny=n, batch=B, K=K, kind=kind, separate_through='parent library' if args.parent_lib else 'this library')
                restore()
                s.step_tangents_scalar(st, dwhat, dthat, 3)
                mine = (dwhat.clone(), dthat.clone(), st.what.clone(), st.that.clone())
                restore()
                separate(3)
                case['shared_bitwise_separate'] = bool(torch.equal(mine[0], dwhat) and torch.equal(mine[1], dthat)
                                                       and all(torch.equal(mine[2], c.what) and torch.equal(mine[3], c.that) for c in clones))
                again = (dwhat.clone(), dthat.clone())
                restore()
                separate(3)
                case['separate_reproduces_itself'] = bool(torch.equal(again[0], dwhat) and torch.equal(again[1], dthat))
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
                    case[name] = stats(ts[name], 1 if name == 'orthonormalize' else steps)
                case['shared_over_separate'] = ratio(ts['shared'], ts['separate'])
                case['separate_again_over_separate'] = aa = ratio(ts['separate_again'], ts['separate'])
                case['shared_faster_by_more_than_the_spread'] = bool(case['shared_over_separate']['max'] < aa['min'])
                case['model_shared_over_separate'] = round((1 + K) / (2.0 * K), 4)
                case['orthonormalize_in_shared_steps'] = round(case['orthonormalize']['ms'] / case['shared']['ms'], 3)
                out.append(case)
                print(json.dumps(case), flush=True)
                del st, clones, dwhat, dthat, w0, t0, saved
                torch.cuda.empty_cache()
    return out


def existing_steps(args, this, parent):
    """The steps the parent has, this build against the parent's under the same direct call: bitwise, and A/B beside A/A."""
    out = []
    K = 4
    for n, BK in CASES:
        B = BK // K
        mk = lambda **kw: PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, **kw).kolmogorov_forcing(4, 1.0)
        flow, sca, buo = mk(), mk(kappa=KAPPA, scalar_gradient=GRAD), mk(kappa=KAPPA, scalar_gradient=GRAD, buoyancy=BUOY)
        u0, v0, th0, dw, dth = fields(n, B, K)
        st = sca.init(u0, v0, th0)
        sca.step(st, 20)
        st.work = torch.empty(max(ops.spec_ns_scalar_tangent_workspace(B, n, n), ops.spec_ns_tangents_workspace(B, K, n, n)), dtype=torch.uint8, device='cuda')
        saved = st.clone()
        fl = flow.init(u0, v0)
        fl.work = st.work
        w0, t0 = sca.init_tangents_scalar(dw, dth)
        dwhat, dthat = w0.clone(), t0.clone()
        steps = args.steps

        def restore():
            st.what.copy_(saved.what)
            st.that.copy_(saved.that)
            fl.what.copy_(saved.what)
            dwhat.copy_(w0)
            dthat.copy_(t0)
        quads = (('scalar', 'scalar', sca, st), ('buoyant', 'buoyant', buo, st), ('tangent', 'tangent', flow, fl), ('tangents', 'tangents', flow, fl),
                 ('scalar_tangent', 'scalar_tangent', sca, st), ('buoyant_tangent', 'scalar_tangent', buo, st))
        case = dict(nx=n, ny=n, batch=B, K_of_tangents=K)
        variants = []
        for name, call, s, state in quads:
            restore()
            this[call](s, state, dwhat, dthat, 3)
            mine = (st.what.clone(), st.that.clone(), fl.what.clone(), dwhat.clone(), dthat.clone())
            restore()
            parent[call](s, state, dwhat, dthat, 3)
            case[name + '_step_bitwise_parent_lib'] = bool(all(torch.equal(a, b) for a, b in zip(mine, (st.what, st.that, fl.what, dwhat, dthat))))
            for tag, calls in (('_parent_lib', parent), ('', this), ('_parent_lib_again', parent)):           # this build's turn between the parent's two
                variants.append((name + '_step_direct' + tag, lambda calls=calls, call=call, s=s, state=state: calls[call](s, state, dwhat, dthat, steps)))
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
        for name, _, _, _ in quads:
            case[name + '_step_direct'] = stats(ts[name + '_step_direct'], steps)
            ab = ratio(ts[name + '_step_direct'], ts[name + '_step_direct_parent_lib'])
            aa = ratio(ts[name + '_step_direct_parent_lib_again'], ts[name + '_step_direct_parent_lib'])
            case[name + '_step_over_parent_lib'], case[name + '_parent_lib_again_over_parent_lib'] = ab, aa
            case[name + '_step_median_inside_parent_lib_noise'] = bool(aa['min'] <= ab['median'] <= aa['max'])
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, saved, fl, dwhat, dthat, w0, t0
        torch.cuda.empty_cache()
    return out


def kernel_resources(path):
    """{kernel: registers, LDS and scratch} of the new kernels from the amdhsa.kernels block that ends a listing of tools/isa_listing.py."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        get = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, blk).group(1))
        if name and any(k in name.group(1) for k in ('PsTangentsScalar', 'ps_row_tans_scalar_kernel', 'ps_tangent_variance_gram')):
            res[name.group(1)] = dict(vgprs=get('vgpr_count'), sgprs=get('sgpr_count'), static_lds_bytes=get('group_segment_fixed_size'),
                                      scratch_bytes=get('private_segment_fixed_size'), vgpr_spills=get('vgpr_spill_count'))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=10, help='steps per timing')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's)")
    ap.add_argument('--isa-listing', default=None, help='pspec_scalar_tangents.s of tools/isa_listing.py (registers, LDS and scratch per kernel)')
    ap.add_argument('--name', default='pspec_scalar_tangents_run', help='the record is OUTDIR/NAME.json')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps)
    this = direct_calls(_lib.LIB_PATH)
    parent = direct_calls(args.parent_lib) if args.parent_lib else None
    rec['timing'] = shared_against_separate(args, (parent or this)['scalar_tangent'])
    rec['existing_steps'] = existing_steps(args, this, parent) if parent else None
    rec['kernels'] = kernel_resources(args.isa_listing)
    import pspec_scalar_lyapunov_cases as SC      # the accuracy figures of tests/test_gpu_pspec_scalar_lyapunov.py and their bounds, kept beside the times
    rec['accuracy'] = dict(measured=SC.MEASURED, bound=SC.BOUND, restatement_at_rest=SC.REST_ORACLE)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, args.name + '.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
