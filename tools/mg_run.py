"""Times the multigrid pressure solve (nns.ops.fd_poisson_mg_) and prints ONE JSON record.

Cases: 64^2 (B = 1, 64), 512^2 (B = 16), 1024^2 (B = 1, 8), float32 and float64, random boundary ring + right-hand side (tests/mg_oracle.py:
random_problem), tol 1e-6, max 30 cycles.  Per case: cycles to tolerance, ms per solve (device events around the whole call, host status reads
included, warmed, median of --reps), ms per cycle, launches per cycle, rel-L2 error of grid 0 against the exact discrete solve; alongside,
red-black SOR (nns.ops.fd_sor_redblack_, beta 1.25, tol 0: all 49 sweeps) on the same grids: its time and the error it leaves.

    python tools/mg_run.py [--reps 5] [--only 1024x1:f32] [--out FILE]

--only restricts the run to one case (for a kernel-trace run: rocprofv3 --kernel-trace --stats -- python tools/mg_run.py --only 1024x1:f32);
--trace-levels TRACE.csv --only NxB:dtype reads that run's kernel_trace.csv and prints the multigrid kernels' time per level (no GPU needed)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import mg_oracle as M  # noqa: E402
from nns import ops  # noqa: E402

CASES = [(64, 1), (64, 64), (512, 16), (1024, 1), (1024, 8)]
LDS_MAX = 150 * 1024


def launches_per_cycle(n, elem):
    """csrc/mg_kernels.hip: per chip-wide level 4 + 4 half-sweeps, restriction, prolongation; ONE tail launch; norm + finish when the finest
    level is chip-wide."""
    levs = M.hierarchy(n, n, *M.spacings(n, n))
    sizes = [a * b for a, b, _, _ in levs]
    mx, my = levs[-1][0] - 2, levs[-1][1] - 2
    tail_elems = lambda l: 2 * sum(sizes[l:]) + mx * mx + my * my + 2 * mx * my
    t = len(levs) - 1
    while t > 0 and tail_elems(t - 1) * elem <= LDS_MAX:
        t -= 1
    return 10 * t + 1 + (2 if t > 0 else 0), t, [l[:2] for l in levs]


def timed(fn, reps, reset):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(2):
        reset()
        fn()
    torch.cuda.synchronize()
    out = None
    for a, b in ev:
        reset()
        a.record()
        out = fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])), out


def run_case(n, B, dt, reps, sor):
    npdt = np.float32 if dt == 'f32' else np.float64
    dx, dy = M.spacings(n, n)
    P, Cs = M.random_problem(n, n, seed=n + B, B=B)
    P, Cs = P.astype(npdt), Cs.astype(npdt)
    p0, C = torch.as_tensor(P, device='cuda'), torch.as_tensor(Cs, device='cuda')
    p = p0.clone()
    reset = lambda: p.copy_(p0)
    ms, info = timed(lambda: ops.fd_poisson_mg_(p, C, dx, dy, tol=1e-6, max_cycles=30), reps, reset)
    info = info.cpu().numpy()
    ex = M.exact_solve(P[0], Cs[0], dx, dy)
    rel = lambda a: float(np.linalg.norm(a.astype(np.float64) - ex) / np.linalg.norm(ex))
    err = rel(p[0].cpu().numpy())
    lpc, tail, levels = launches_per_cycle(n, p.element_size())
    cyc = info[:, 0]
    rec = dict(n=n, batch=B, dtype=dt, levels=levels, tail_level=tail, cycles_max=int(cyc.max()), cycles_min=int(cyc.min()),
               ratio_max=float(info[:, 1].max()), ms_per_solve=ms, ms_per_cycle=ms / max(1, int(cyc.max())), launches_per_cycle=lpc,
               rel_l2_vs_exact=err)
    if sor:
        ms_rb, _ = timed(lambda: ops.fd_sor_redblack_(p, C, dx, dy, 1.25, 0.0, 49), reps, reset)
        rec['redblack_49'] = dict(ms_per_solve=ms_rb, rel_l2_vs_exact=rel(p[0].cpu().numpy()))
    return rec


def trace_levels(path, n, B, elem):
    """Per-level sums of a rocprofv3 kernel trace of the solve: each launch is mapped to its level by its grid (the launch geometry of
    csrc/mg_kernels.hip)."""
    import csv
    _, tail, levels = launches_per_cycle(n, elem)
    geo = {}
    for l, (nx, ny) in enumerate(levels):
        gx = ((ny - 1) // 2 + 255) // 256
        geo[('mg_smooth', gx * 256, min(nx - 2, max(1, 2048 // (gx * B))))] = l
        geo[('mg_prolong', -(-((nx - 2) * (ny - 2)) // 256) * 256, 1)] = l
        if l > 0:
            geo[('mg_restrict', -(-(nx * ny) // 256) * 256, 1)] = l - 1           # labelled by the fine level it restricts from
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r['Kernel_Name']
        if 'mg_' not in name:
            continue
        short = name[name.index('mg_'):].split('_kernel')[0]
        key = (short, int(r['Grid_Size_X']), int(r['Grid_Size_Y']))
        lev = geo.get(key, 'tail' if short == 'mg_tail' else 'finest' if short in ('mg_norm', 'mg_finish', 'mg_init') else '?')
        if isinstance(lev, int):
            lev = '%dx%d' % tuple(levels[lev])
        d = rows.setdefault((lev, short), [0, 0.0])
        d[0] += 1
        d[1] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3
    out = [dict(level=k[0], kernel=k[1], launches=v[0], total_us=round(v[1], 1), mean_us=round(v[1] / v[0], 2)) for k, v in sorted(rows.items(), key=lambda kv: -kv[1][1])]
    return dict(tool='mg_run --trace-levels', case='%dx%d' % (n, B), tail_level='%dx%d' % tuple(levels[tail]), rows=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', default=None, help='NxB:dtype, e.g. 1024x1:f32')
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-levels', default=None, metavar='KERNEL_TRACE_CSV')
    a = ap.parse_args()
    if a.trace_levels:
        nb, dt = a.only.split(':')
        n, B = map(int, nb.split('x'))
        print(json.dumps(trace_levels(a.trace_levels, n, B, 4 if dt == 'f32' else 8), indent=1))
        return
    torch.cuda.set_device(0)
    cases = [(n, B, dt) for n, B in CASES for dt in ('f32', 'f64')]
    if a.only:
        nb, dt = a.only.split(':')
        n, B = map(int, nb.split('x'))
        cases = [(n, B, dt)]
    recs = [run_case(n, B, dt, a.reps, sor=not a.only) for n, B, dt in cases]
    out = dict(tool='mg_run', device=torch.cuda.get_device_name(0), tol=1e-6, max_cycles=30, cases=recs)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
