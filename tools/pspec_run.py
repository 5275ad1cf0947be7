"""Times the pseudo-spectral periodic solver's fused step (nns.periodic.PeriodicSolver.step: 8 launches of csrc/pspec_kernels.hip per step)
against a COMPOSED step of the same scheme on the same inputs in the same run: the standalone transforms nns.ops.spec_rfft2 /
spec_irfft2 plus torch elementwise ops on full rfft2-layout spectra.  Writes ONE JSON record to OUTDIR/pspec_run.json and prints it.

    python tools/pspec_run.py OUTDIR [--steps 20] [--reps 5]
    python tools/pspec_run.py OUTDIR --forced [--steps 20] [--reps 7] [--commit ID]
    python tools/pspec_run.py OUTDIR --scalar [--steps 100] [--reps 7] [--commit ID]

Cases: 256^2 x B = 64 and 1024^2 x B = 8, |m| <= 8 initial condition (tests/pspec_oracle.py: random_ic), nu = 1e-3.  Per case: ms per
step of each (device events around `steps` steps, warmed, median of `reps`), the bytes-per-point model of each (below) and the rel-L2
difference of the two after `steps` steps (same scheme, float32 both: rounding only).

--forced instead times the forced step (Kolmogorov force k = 4, drag 0.1: nns_spec_ns_step_forced_f32) next to the unforced step of the
same build on the same state, the three variants (unforced, shared force, per-grid force) taking turns within every repetition, and one
diagnostics call next to one fields call (256^2 x 64 and 1024^2 x 1).  Writes ONE record to OUTDIR/pspec_forced_run.json: per variant the
median ms per step and the spread (max - min) / median over the repetitions, the ratios to the unforced step and the byte model's 54 / 50.

--scalar times the step with a passive scalar (nns_spec_ns_step_scalar_f32: kappa = 1e-3, G = (0.7, -0.4)) next to the flow-only step of the
same build from the same initial state: flow only, scalar over the unforced flow and scalar under the Kolmogorov force and drag take turns
within every repetition.  Per case the median ms per step and spread of each, the ratios to the flow-only step next to the byte model's
84 / 50 and the transform count's 13 / 8, and whether the vorticity spectrum after the timed steps is bitwise the flow-only one; then one
scalar_diagnostics call and one scalar call.  Writes ONE record to OUTDIR/pspec_scalar_run.json.  With --commit the record also holds the
flow-only step against the figure the parent commit recorded in profiles/pspec_forced_run.json (another run: compare within the spreads)."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pspec_oracle as O  # noqa: E402
from nns import ops  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402

CASES = [(256, 64), (1024, 8)]


def fused_bytes_per_point(nx, ny):
    """HBM bytes per grid point per step of the fused step, c = one compacted complex field (8 my1 bytes per row of ny points).
    Per stage the row launch reads 4c (u, v, w_x, w_y) and writes c (the product's kept spectrum); the column launch reads c, moves
    W / A (2c, 3c, 3c, 2c for stages 1..4) and writes the next stage's 4c.  Per step: 20c + 4c + 10c + 16c = 50c."""
    return 50 * 8.0 * ops.spec_ns_kept_y(ny) / ny


def composed_bytes_per_point(nx, ny):
    """The composed step, f = one full rfft2 spectrum (8 (ny/2 + 1) bytes per row), r = one real field (4 ny bytes per row), tables ignored.
    Per evaluation of N: psi (2f), the four spectra (8f), their stack (8f), spec_irfft2's scratch copy (8f), column pass (8f), row pass
    (4f + 4r), the product (9r), spec_rfft2 (3f + r), the mask (2f): 43f + 14r.  Lawson combinations per step: 31f."""
    f, r = 8.0 * (ny // 2 + 1) / ny, 4.0
    return 4 * (43 * f + 14 * r) + 31 * f


class Composed(object):
    """The scheme of tests/pspec_oracle.py on full rfft2-layout complex64 spectra [B, nx, ny/2+1]."""

    def __init__(self, s, what, mean):
        nx, ny, dev = s.nx, s.ny, what.device
        kx, ky, k2, M, ik2 = O.grid(nx, ny, s.Lx, s.Ly)
        t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
        self.s, self.ny = s, ny
        self.ikx, self.iky = t(1j * kx * np.ones_like(k2), torch.complex64), t(1j * ky * np.ones_like(k2), torch.complex64)
        self.M, self.ik2 = t(M), t(ik2)
        self.E, self.E2 = t(np.exp(-s.nu * k2 * s.dt / 2)), t(np.exp(-s.nu * k2 * s.dt))
        B = what.shape[0]
        full = torch.zeros(B, nx, ny // 2 + 1, dtype=torch.complex64, device=dev)
        full[:, :, :s.my1] = torch.view_as_complex(what).transpose(1, 2)
        self.w = full
        self.m0 = (mean * float(nx * ny)).to(torch.complex64)

    def N(self, w):
        psi = w * self.ik2
        uh, vh = self.iky * psi, -self.ikx * psi
        uh[:, 0, 0], vh[:, 0, 0] = self.m0[:, 0], self.m0[:, 1]
        four = torch.stack([uh, vh, self.ikx * w, self.iky * w]).reshape(-1, w.shape[1], w.shape[2])
        phys = ops.spec_irfft2(four, self.ny).view(4, *w.shape[:2], self.ny)
        prod = phys[0] * phys[2] + phys[1] * phys[3]
        return -self.M * ops.spec_rfft2(prod)

    def step(self, nsteps):
        dt, E, E2 = self.s.dt, self.E, self.E2
        w = self.w
        for _ in range(nsteps):
            a = self.N(w)
            b = self.N(E * (w + dt / 2 * a))
            c = self.N(E * w + dt / 2 * b)
            d = self.N(E2 * w + dt * E * c)
            w = E2 * w + dt / 6 * (E2 * a + 2 * E * (b + c) + d)
        self.w = w


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts, per=1):
    med = float(np.median(ts))
    return dict(ms=round(med / per, 5), spread=round((max(ts) - min(ts)) / med, 4))


def forced_main(args):
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps,
               byte_model_ratio=round(54 / 50, 3), cases=[], diagnostics=[])
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device='cuda')
    for n, B in CASES:
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        fx, fy = O.random_ic(B, n, n, 8, seed=n + B + 1, umax=1.0)
        plain = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3)
        shared = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1).kolmogorov_forcing(4, 1.0)
        per_grid = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1).set_forcing(dev(fx), dev(fy))
        st = plain.init(dev(u0), dev(v0))
        w0 = st.what.clone()
        variants = [('unforced', plain), ('forced_shared', shared), ('forced_per_grid', per_grid)]
        ts = {name: [] for name, _ in variants}
        for name, s in variants:                                  # warm every kernel of every variant
            s.step(st, 2)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, s in variants:
                st.what.copy_(w0)
                ts[name].append(event_ms(lambda: s.step(st, args.steps)))
        case = dict(nx=n, ny=n, batch=B)
        for name, _ in variants:
            case[name] = stats(ts[name], args.steps)
        for name in ('forced_shared', 'forced_per_grid'):
            case[name + '_over_unforced'] = round(case[name]['ms'] / case['unforced']['ms'], 4)
        rec['cases'].append(case)
        print(json.dumps(case), flush=True)
        del st
        torch.cuda.empty_cache()
    for n, B in ((256, 64), (1024, 1)):
        s = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1).kolmogorov_forcing(4, 1.0)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        st = s.init(dev(u0), dev(v0))
        out = tuple(torch.empty(B, n, n, device='cuda') for _ in range(3))
        s.diagnostics(st), s.fields(st, out=out)
        torch.cuda.synchronize()
        td, tf = [], []
        for _ in range(args.reps):
            td.append(event_ms(lambda: [s.diagnostics(st) for _ in range(10)]))
            tf.append(event_ms(lambda: [s.fields(st, out=out) for _ in range(10)]))
        d = dict(nx=n, ny=n, batch=B, diagnostics=stats(td, 10), fields=stats(tf, 10))
        rec['diagnostics'].append(d)
        print(json.dumps(d), flush=True)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_forced_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def scalar_main(args):
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps,
               byte_model_ratio=round(84 / 50, 3), byte_model_ratio_forced=round(88 / 50, 3), transform_ratio=round(13 / 8, 3), cases=[], calls=[])
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device='cuda')
    kw = dict(kappa=1e-3, scalar_gradient=(0.7, -0.4))
    for n, B in CASES:
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0)[0] + 0.5
        plain = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, **kw)
        forced = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1, **kw).kolmogorov_forcing(4, 1.0)
        flow = plain.init(dev(u0), dev(v0))
        both = plain.init(dev(u0), dev(v0), dev(th0))
        w0, t0 = both.what.clone(), both.that.clone()
        variants = [('flow_only', plain, flow), ('scalar', plain, both), ('scalar_forced', forced, both)]
        ts = {name: [] for name, _, _ in variants}
        for name, s, st in variants:                              # warm every kernel of every variant
            s.step(st, 2)
        torch.cuda.synchronize()
        ends = {}
        for _ in range(args.reps):
            for name, s, st in variants:
                st.what.copy_(w0)
                if st.that is not None:
                    st.that.copy_(t0)
                ts[name].append(event_ms(lambda: s.step(st, args.steps)))
                ends[name] = st.what.clone()
        case = dict(nx=n, ny=n, batch=B)
        for name, _, _ in variants:
            case[name] = stats(ts[name], args.steps)
        for name in ('scalar', 'scalar_forced'):
            case[name + '_over_flow_only'] = round(case[name]['ms'] / case['flow_only']['ms'], 4)
        case['what_bitwise_flow_only'] = bool(torch.equal(ends['flow_only'], ends['scalar']))
        c = 8.0 * ops.spec_ns_kept_y(n) * n * B                           # bytes of one compacted complex field of the batch
        case['scalar_GBps_on_84c'] = round(84 * c / case['scalar']['ms'] / 1e6, 1)
        if args.commit != 'unknown':
            parent = json.load(open(os.path.join(ROOT, 'profiles', 'pspec_forced_run.json')))
            pc = [x for x in parent['cases'] if (x['nx'], x['batch']) == (n, B)][0]['unforced']
            case['flow_only_parent_record'] = dict(commit=parent['commit'], steps=parent['steps'], **pc)
            case['flow_only_over_parent_record'] = round(case['flow_only']['ms'] / pc['ms'], 4)
        rec['cases'].append(case)
        print(json.dumps(case), flush=True)
        del flow, both, ends
        torch.cuda.empty_cache()
    for n, B in ((256, 64), (1024, 1)):
        s = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, **kw)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        st = s.init(dev(u0), dev(v0), dev(u0 + 0.5))
        out = torch.empty(B, n, n, device='cuda')
        s.scalar_diagnostics(st), s.scalar(st, out=out)
        torch.cuda.synchronize()
        td, tf = [], []
        for _ in range(args.reps):
            td.append(event_ms(lambda: [s.scalar_diagnostics(st) for _ in range(10)]))
            tf.append(event_ms(lambda: [s.scalar(st, out=out) for _ in range(10)]))
        d = dict(nx=n, ny=n, batch=B, scalar_diagnostics=stats(td, 10), scalar=stats(tf, 10))
        rec['calls'].append(d)
        print(json.dumps(d), flush=True)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_scalar_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=None, help='steps per timing (default 20; 100 with --scalar)')
    ap.add_argument('--reps', type=int, default=None)
    ap.add_argument('--forced', action='store_true', help='time the forced step and the diagnostics instead (see the module note)')
    ap.add_argument('--scalar', action='store_true', help='time the step with a passive scalar instead (see the module note)')
    ap.add_argument('--commit', default='unknown', help='recorded in the --forced and --scalar records')
    args = ap.parse_args()
    if args.forced and args.scalar:
        ap.error('--forced and --scalar are two runs')
    if args.reps is None:
        args.reps = 7 if args.forced or args.scalar else 5
    if args.steps is None:
        args.steps = 100 if args.scalar else 20
    torch.cuda.set_device(0)
    if args.forced:
        return forced_main(args)
    if args.scalar:
        return scalar_main(args)
    rec = dict(device=torch.cuda.get_device_name(0), steps=args.steps, reps=args.reps, cases=[])
    for n, B in CASES:
        s = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        st = s.init(torch.as_tensor(u0, dtype=torch.float32, device='cuda'), torch.as_tensor(v0, dtype=torch.float32, device='cuda'))
        comp = Composed(s, st.what, st.mean)
        w0 = st.what.clone()
        # agreement: the same number of steps from the same state
        s.step(st, args.steps)
        comp.step(args.steps)
        uf = s.fields(st)[0]
        cw = comp.w[:, :, :s.my1].transpose(1, 2).contiguous()
        st.what.copy_(torch.view_as_real(cw))
        uc = s.fields(st)[0]
        diff = float((uf - uc).norm() / uc.norm())
        st.what.copy_(w0)
        ms_fused = timed(lambda: s.step(st, args.steps), args.reps) / args.steps
        ms_comp = timed(lambda: comp.step(args.steps), args.reps) / args.steps
        case = dict(nx=n, ny=n, batch=B, ms_per_step_fused=round(ms_fused, 4), ms_per_step_composed=round(ms_comp, 4),
                    speedup=round(ms_comp / ms_fused, 2),
                    bytes_per_point_fused=round(fused_bytes_per_point(n, n), 1),
                    bytes_per_point_composed=round(composed_bytes_per_point(n, n), 1),
                    fused_GBps=round(fused_bytes_per_point(n, n) * n * n * B / ms_fused / 1e6, 1),
                    rel_l2_fused_vs_composed_u=float('%.3g' % diff))
        rec['cases'].append(case)
        print(json.dumps(case), flush=True)
        del st, comp
        torch.cuda.empty_cache()
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
