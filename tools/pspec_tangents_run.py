"""Measures K tangents on one base of the periodic spectral solver (nns.periodic.PeriodicSolver.step_tangents: nns_spec_ns_step_tangents_f32
of csrc/pspec_kernels.hip) against K calls of the single-tangent step, and the cost of one orthonormalisation.  Writes ONE JSON record to
OUTDIR/pspec_tangents_run.json and prints it.

    python tools/pspec_tangents_run.py OUTDIR [--steps 20] [--reps 7] [--commit ID] [--parent-lib PATH] [--name NAME] [--isa-notes FILE]

Timing: at 256^2 with B K = 64 and 1024^2 with B K = 8, for K = 2, 4, 8 (|m| <= 8 flow and perturbations, Kolmogorov force k = 4, drag 0.1),
these take turns within every repetition, each from the same saved state: one step_tangents call with K tangents on B grids; K calls of
nns_spec_ns_step_tangent_f32 on K clones of the state, one member each -- with --parent-lib through another build of the library (the parent
commit's) loaded into the same process, else through this build, under the same direct call -- and that sequence once more, so that the
ratio of its two turns is the noise the shared / separate ratio is read against.  Also whether the shared call's members and base are the
bits of the separate calls.  A timing is device events around the work, reported per step as the median over the repetitions with the spread
(max - min) / median; ratios are medians of the per-repetition ratios.  One orthonormalize_tangents is timed in the same turns and given in
units of one shared step.

The byte model to compare against, in compacted fields c moved per step: the flow's step moves 50c and every tangent
50c more, but the base's share is moved once per call: (50 + 50 K) c shared against 100 K c separate, (1 + K) / (2 K).
The register and scratch figures of the new kernels come from the code object's metadata (--isa-notes FILE: the text of `llvm-readelf
--notes` on the library, or the amdhsa.kernels block that ends the listing of tools/isa_listing.py, made at build time)."""
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
from nns import _lib  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402
from pspec_adjoint_run import event_ms, stats, ratio, dev  # noqa: E402

CASES = [(256, 64), (1024, 8)]            # (n, B K)
KS = (2, 4, 8)
DT, NU, DRAG = 1e-3, 1e-3, 0.1


def single_tangent_call(path):
    """nns_spec_ns_step_tangent_f32 of a build of the library, under the argument list of include/nns.h."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_tangent_f32.argtypes = [P] * 4 + [I, P, I, P, Z] + [I] * 3 + [D] * 5 + [P, P, ctypes.c_uint64, P, P, I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def call(s, st, dwhat, n):
        rc = L.nns_spec_ns_step_tangent_f32(p(st.what), p(dwhat), p(st.mean), p(s.ghat), 1, None, 0, p(st.work), st.work.numel(), st.batch, s.nx,
                                            s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, None, None, 0, None, None, n, stream())
        if rc != 0:
            raise RuntimeError('the library refused the call: %d' % rc)
    return call


def timing(args):
    out = []
    single = single_tangent_call(args.parent_lib or _lib.LIB_PATH)
    for n, BK in CASES:
        for K in KS:
            B = BK // K
            s = PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG).kolmogorov_forcing(4, 1.0)
            u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
            dw0 = [O.random_ic(B, n, n, 8, seed=n + B + 2 + k, umax=1.0)[0] for k in range(K)]
            st = s.init(dev(u0), dev(v0))
            s.step(st, 20)                                                # a developed state
            saved = st.what.clone()
            d0 = s.init_tangents(torch.stack([dev(a) for a in dw0]))
            s.orthonormalize_tangents(d0)
            dwhat = d0.clone()
            s.step_tangents(st, dwhat, 1)                                 # grows the workspace
            clones = [st.clone() for _ in range(K)]
            for c in clones:
                c.work = torch.empty_like(st.work)
            steps = args.steps

            def restore():
                st.what.copy_(saved)
                dwhat.copy_(d0)
                for c in clones:
                    c.what.copy_(saved)

            def separate():
                for k, c in enumerate(clones):
                    single(s, c, dwhat[k], steps)
            variants = [('separate', separate), ('shared', lambda: s.step_tangents(st, dwhat, steps)), ('separate_again', separate),
                        ('orthonormalize', lambda: s.orthonormalize_tangents(dwhat))]
            case = dict(nx=n, ny=n, batch=B, K=K, separate_through='parent library' if args.parent_lib else 'this library')
            restore()
            s.step_tangents(st, dwhat, 3)
            mine = (dwhat.clone(), st.what.clone())
            restore()
            for k, c in enumerate(clones):
                single(s, c, dwhat[k], 3)
            case['shared_bitwise_separate'] = bool(torch.equal(mine[0], dwhat) and all(torch.equal(mine[1], c.what) for c in clones))
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
            del st, clones, dwhat, d0, saved
            torch.cuda.empty_cache()
    return out


def kernel_resources(path):
    """{kernel: (vgprs, scratch bytes)} of the new kernels from the text of `llvm-readelf --notes` on the library."""
    if not path or not os.path.exists(path):
        return None
    res = {}
    for blk in open(path).read().split('- .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        vg, sc = re.search(r'\.vgpr_count:\s+(\d+)', blk), re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
        if name and vg and sc and any(k in name.group(1) for k in ('PsTangents', 'ps_row_tans_kernel', 'ps_tangent_gram', 'ps_tangent_combine')):
            res[name.group(1)] = dict(vgprs=int(vg.group(1)), scratch_bytes=int(sc.group(1)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=20, help='steps per timing')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's) for the K separate calls")
    ap.add_argument('--isa-notes', default=None, help='text of llvm-readelf --notes on libnns_hip.so (registers and scratch per kernel)')
    ap.add_argument('--name', default='pspec_tangents_run', help='the record is OUTDIR/NAME.json')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps)
    rec['timing'] = timing(args)
    rec['kernels'] = kernel_resources(args.isa_notes)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, args.name + '.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
