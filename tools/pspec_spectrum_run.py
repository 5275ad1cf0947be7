"""Times the shell spectra and spectral transfers of the periodic spectral solver (nns.periodic.PeriodicSolver.spectrum / transfer:
nns_spec_ns_spectrum_f32, nns_spec_ns_transfer_f32 of csrc/pspec_kernels.hip) and, in the same run on the same states, what they are to be read
against: the per-grid totals (``diagnostics``: one workgroup per grid), one time step, and the same energy and enstrophy spectra COMPOSED from
``fields()``, torch FFTs and ``index_add_``.  Writes ONE JSON record to OUTDIR/pspec_spectrum_run.json and prints it.

    python tools/pspec_spectrum_run.py OUTDIR [--calls 20] [--reps 9] [--commit ID]

Cases: 256^2 x 64, 1024^2 x 8 and 1024^2 x 1, |m| <= 8 flow and scalar (tests/pspec_oracle.py: random_ic), Kolmogorov force k = 4, drag 0.1,
kappa = 1e-3.  Every variant is warmed (code objects, LDS attributes, FFT plans), then the variants take turns within every repetition; a
timing is device events around `calls` calls (a step: `calls` steps), reported per call as the median over the repetitions with the spread
(max - min) / median.  Per case also: the bytes the spectrum has to read (the stored spectra of the flow and the scalar once, the shared force
once) and the rate that gives, and the agreement of the composed spectrum with the kernel's (float32 transforms
against float64 sums of the state: rounding only)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pspec_oracle as O  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402

CASES = [(256, 64), (1024, 8), (1024, 1)]


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts, per):
    med = float(np.median(ts))
    return dict(ms=round(med / per, 5), spread=round((max(ts) - min(ts)) / med, 4))


class Composed(object):
    """E(s), Z(s) [B, S] from the physical fields: fields(), two torch rfft2, the Parseval weights and index_add_ over the shell index."""

    def __init__(self, s, B):
        nx, ny = s.nx, s.ny
        k, dk = s.shells()
        kx, ky, k2, M, ik2 = O.grid(nx, ny, s.Lx, s.Ly)
        wt = np.where(np.arange(ny // 2 + 1) == 0, 1.0, 2.0)[None, :] * M          # the kept modes; the Nyquist column is outside the band
        self.s, self.S = s, len(k)
        self.idx = torch.as_tensor(np.minimum(np.floor(np.sqrt(k2) / dk + 0.5), len(k) - 1).astype(np.int64).ravel(), device='cuda')
        self.wt = torch.as_tensor((0.5 * wt / float(nx * ny) ** 2).ravel(), dtype=torch.float64, device='cuda')
        self.k2 = torch.as_tensor(k2.ravel(), dtype=torch.float64, device='cuda')
        self.out = tuple(torch.empty(B, nx, ny, device='cuda') for _ in range(3))

    def __call__(self, st):
        u, v, _ = self.s.fields(st, out=self.out)
        uh, vh = torch.fft.rfft2(u), torch.fft.rfft2(v)
        e = ((uh.real.double() ** 2 + uh.imag.double() ** 2 + vh.real.double() ** 2 + vh.imag.double() ** 2).flatten(1)) * self.wt
        E = torch.zeros(e.shape[0], self.S, dtype=torch.float64, device='cuda').index_add_(1, self.idx, e)
        Z = torch.zeros(e.shape[0], self.S, dtype=torch.float64, device='cuda').index_add_(1, self.idx, e * self.k2)
        return E, Z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--calls', type=int, default=20, help='calls per timed window')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--commit', default='unknown')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, calls=args.calls, reps=args.reps,
               cases=[])
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device='cuda')
    for n, B in CASES:
        s = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1, kappa=1e-3, scalar_gradient=(0.7, -0.4)).kolmogorov_forcing(4, 1.0)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0)[0] + 0.5
        st = s.init(dev(u0), dev(v0), dev(th0))
        s.step(st, 20)                                                    # a developed state; also warms the step
        flow = s.init(dev(u0), dev(v0))
        flow.what.copy_(st.what)
        comp = Composed(s, B)
        variants = [('spectrum', lambda: s.spectrum(st)), ('spectrum_flow_only', lambda: s.spectrum(flow)),
                    ('transfer', lambda: s.transfer(st)), ('transfer_flow_only', lambda: s.transfer(flow)),
                    ('diagnostics', lambda: s.diagnostics(st)), ('scalar_diagnostics', lambda: s.scalar_diagnostics(st)),
                    ('composed_spectrum', lambda: comp(flow)), ('step', lambda: s.step(st, 1))]
        for _, fn in variants:                                            # warm every variant
            fn(), fn()
        torch.cuda.synchronize()
        # agreement of the composed spectrum with the kernel's, and of the kernel's sums with the totals, on the state that is timed
        sp, (cE, cZ) = s.spectrum(flow), comp(flow)
        d = s.diagnostics(flow)
        case = dict(nx=n, ny=n, batch=B, shells=len(sp.k),
                    composed_vs_kernel=dict(E=float(((cE - sp.energy).abs().sum(-1) / sp.energy.sum(-1)).max()),
                                            Z=float(((cZ - sp.enstrophy).abs().sum(-1) / sp.enstrophy.sum(-1)).max())),
                    shell_sums_vs_diagnostics=dict(E=float((sp.energy.sum(-1) / d.energy - 1).abs().max()),
                                                   Z=float((sp.enstrophy.sum(-1) / d.enstrophy - 1).abs().max())))
        ts = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                ts[name].append(event_ms(fn, args.calls))
        for name, _ in variants:
            case[name] = stats(ts[name], args.calls)
        c = 8.0 * s.my1 * n                                               # bytes of one stored spectrum of one grid
        case['spectrum_bytes'] = int(c * (2 * B + 1))                     # w^ and theta^ of every grid, the shared g^ once
        case['spectrum_GBps'] = round(case['spectrum_bytes'] / case['spectrum']['ms'] / 1e6, 1)
        case['diagnostics_GBps'] = round(c * (B + 1) / case['diagnostics']['ms'] / 1e6, 1)
        for name in ('spectrum', 'transfer', 'composed_spectrum', 'diagnostics'):
            case[name + '_over_step'] = round(case[name]['ms'] / case['step']['ms'], 4)
        case['composed_over_spectrum_flow_only'] = round(case['composed_spectrum']['ms'] / case['spectrum_flow_only']['ms'], 2)
        rec['cases'].append(case)
        print(json.dumps(case), flush=True)
        del st, flow, comp
        torch.cuda.empty_cache()
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_spectrum_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
