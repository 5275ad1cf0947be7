"""Measures the Boussinesq buoyancy of the periodic spectral solver (nns.periodic.PeriodicSolver with buoyancy: nns_spec_ns_step_buoyant_f32,
nns_spec_ns_fields_buoyant_f32, nns_spec_ns_buoyancy_spectrum_f32 of csrc/pspec_kernels.hip).  Writes ONE JSON record to
OUTDIR/pspec_buoyant_run.json and prints it.

    python tools/pspec_buoyant_run.py OUTDIR [--steps 100] [--reps 7] [--commit ID] [--parent-lib PATH] [--no-accuracy]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow and scalar, Kolmogorov force k = 4, drag 0.1, kappa = 1e-3, G = (0.7, -0.4), b = (0.3, 1.2))
the buoyant, passive-scalar and flow-only steps take turns within every repetition, each from the same saved state (restored outside the timed
window); with --parent-lib also the passive step of another build of the library (the parent commit's), loaded into the same process and called
on the same buffers.  A timing is device events around one call of `steps` steps, reported per step as the median over the repetitions with the
spread (max - min) / median; the ratios are medians of the per-repetition ratios.  Also one buoyancy_spectrum call and one buoyant fields call
(against the flow's own fields call).
Accuracy (tests/pspec_buoyant_cases.py, the figures tests/test_gpu_pspec_buoyant.py bounds): the five full-band cases after 12 steps against the
float64 restatement -- rel-L2 of what, that', u, v and the buoyant pressure -- and the four analytic plane waves after 200 steps."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pspec_oracle as O  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402

CASES = [(256, 64), (1024, 8)]
GRAD, BUOY = (0.7, -0.4), (0.3, 1.2)


def event_ms(fn, calls=1):
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


def ratio(a, b):
    r = np.array(a) / np.array(b)
    return dict(median=round(float(np.median(r)), 4), min=round(float(r.min()), 4), max=round(float(r.max()), 4))


def dev(a):
    return torch.as_tensor(np.array(a), dtype=torch.float32, device='cuda')


def parent_scalar_step(path):
    """The passive step of another build of the library: nns_spec_ns_step_scalar_f32 through its own ctypes handle."""
    L = ctypes.CDLL(path)
    f = L.nns_spec_ns_step_scalar_f32
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_int] * 3 + [ctypes.c_double] * 8 + [ctypes.c_int,
                                                                                                                                        ctypes.c_void_p]
    f.restype = ctypes.c_int

    def step(s, st, nsteps):
        rc = f(st.what.data_ptr(), st.that.data_ptr(), st.mean.data_ptr(), s.ghat.data_ptr(), int(s.ghat.shape[0]), st.work.data_ptr(), st.work.numel(),
               st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa, s.scalar_gradient[0], s.scalar_gradient[1], nsteps,
               torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('the parent library refused the step: %d' % rc)
    return step


def timing(args):
    out = []
    parent = parent_scalar_step(args.parent_lib) if args.parent_lib else None
    for n, B in CASES:
        mk = lambda b: PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1, kappa=1e-3, scalar_gradient=GRAD, buoyancy=b).kolmogorov_forcing(4, 1.0)
        sb, sp = mk(BUOY), mk((0.0, 0.0))
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 2, umax=1.0)[0] + 0.5
        st = sb.init(dev(u0), dev(v0), dev(th0))
        sb.step(st, 20)                                                   # a developed state
        saved = st.clone()
        flow = sb.init(dev(u0), dev(v0))

        def restore():
            st.what.copy_(saved.what), st.that.copy_(saved.that), flow.what.copy_(saved.what)

        variants = [('buoyant', lambda: sb.step(st, args.steps)), ('passive', lambda: sp.step(st, args.steps)),
                    ('flow_only', lambda: sb.step(flow, args.steps))]
        if parent:
            variants.append(('passive_parent_lib', lambda: parent(sp, st, args.steps)))
        case = dict(nx=n, ny=n, batch=B)
        if parent:                                                        # the same instructions: the same bits
            restore()
            sp.step(st, 3)
            mine = (st.what.clone(), st.that.clone())
            restore()
            parent(sp, st, 3)
            case['passive_bitwise_parent_lib'] = bool(torch.equal(mine[0], st.what) and torch.equal(mine[1], st.that))
        for _, fn in variants:                                            # warm every variant
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
            case[name] = stats(ts[name], args.steps)
        case['buoyant_over_passive'] = ratio(ts['buoyant'], ts['passive'])
        case['passive_over_flow_only'] = ratio(ts['passive'], ts['flow_only'])
        if parent:
            case['passive_over_parent_lib'] = ratio(ts['passive'], ts['passive_parent_lib'])
        restore()
        outs = tuple(torch.empty(B, n, n, device='cuda') for _ in range(3))
        calls = [('buoyancy_spectrum', lambda: sb.buoyancy_spectrum(st)), ('fields_buoyant', lambda: sb.fields(st, out=outs)),
                 ('fields_flow_only', lambda: sb.fields(flow, out=outs))]
        for _, fn in calls:
            fn(), fn()
        torch.cuda.synchronize()
        tc = {name: [event_ms(fn, 10) for _ in range(args.reps)] for name, fn in calls}
        for name, _ in calls:
            case[name] = stats(tc[name], 10)
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, saved, flow, outs
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_buoyant_cases as BC
    import pspec_buoyant_oracle as BO
    import pspec_cases as C
    import pspec_forced_cases as FC
    host = lambda t: t.cpu().numpy().astype(np.float64)
    cplx = lambda t: host(t)[..., 0] + 1j * host(t)[..., 1]
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
    full, waves = [], []
    for case in BC.CASES:
        nx, ny, B, Lx, Ly, _ = case
        S, u0, v0, th0, w, t, mean = BC.reference(case)
        s = PeriodicSolver(nx, ny, S.dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=FC.DRAG, kappa=BC.KAPPA, scalar_gradient=BC.GRAD,
                           buoyancy=BC.BUOY).kolmogorov_forcing(FC.KF, FC.AMP)
        st = s.init(dev(u0), dev(v0), dev(th0))
        s.step(st, BC.NSTEPS)
        u, v, p = (host(f) for f in s.fields(st))
        ru, rv, rp = S.fields(w, mean, t)
        r = dict(nx=nx, ny=ny, batch=B, steps=BC.NSTEPS, what=rel(cplx(st.what), S.compact(w)),
                 that_fluct=rel(S.compact(S.fluctuation(S.expand(cplx(st.that)))), S.compact(S.fluctuation(t))),
                 mean_theta=float(np.abs(cplx(st.that)[:, 0, 0].real - t[..., 0, 0].real).max() / (nx * ny)),
                 u=rel(u, ru), v=rel(v, rv), p=rel(p, rp), p_flow_only_vs_buoyant=rel(S.fields(w, mean)[2], rp))
        bs, bp = s.buoyancy_spectrum(st).cpu().numpy(), s.buoyancy_power(st).cpu().numpy()
        own = S.buoyancy_spectrum(S.expand(cplx(st.what)), S.expand(cplx(st.that)))
        r['buoyancy_spectrum_sum_vs_power'] = float(np.abs(bs.sum(-1) / bp - 1).max())
        r['buoyancy_spectrum_vs_oracle_sums'] = float((np.abs(bs - own).max(-1) / np.abs(own).max(-1)).max())
        full.append({k: (float('%.3e' % x) if isinstance(x, float) else x) for k, x in r.items()})
        print(json.dumps(full[-1]), flush=True)
    for wave in BC.WAVES:
        nx, ny, Lx, Ly, m, b, G, nu, dt = wave
        n, U = BC.WAVE_STEPS, BC.wave_flow(G)
        s = PeriodicSolver(nx, ny, dt, C.RHO, nu, Lx=Lx, Ly=Ly, kappa=nu, scalar_gradient=G, buoyancy=b)
        u0, v0, _, th0 = BO.plane_wave(nx, ny, 0.0, m, b, G, U, nu, Lx, Ly)[:4]
        st = s.init(dev(u0), dev(v0), dev(th0))
        s.step(st, n)
        _, _, rw, rt, aw, at, om = BO.plane_wave(nx, ny, n * dt, m, b, G, U, nu, Lx, Ly)
        S = BO.BuoyantScheme(nx, ny, dt, C.RHO, nu, Lx, Ly, kappa=nu, grad=G, buoy=b)
        wf, th = S.irfft2(S.expand(cplx(st.what)))[0], host(s.scalar(st))[0]
        waves.append(dict(nx=nx, ny=ny, m=list(m), b=list(b), G=list(G), steps=n, amplitude_w=round(float(aw), 4), amplitude_theta=round(float(at), 5),
                          w=float('%.3e' % (np.abs(wf - rw).max() / aw)),
                          theta_fluct=float('%.3e' % (np.abs((th - th.mean()) - (rt - rt.mean())).max() / at)), mean_theta=float('%.1e' % th.mean()),
                          rk4_bound=float('%.2e' % BC.wave_rk4_error(wave, U))))
        print(json.dumps(waves[-1]), flush=True)
    return dict(full_band=full, plane_waves=waves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=100, help='steps per timing')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's) for the same-process A/B")
    ap.add_argument('--no-accuracy', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps, buoyancy=list(BUOY), gradient=list(GRAD))
    if not args.no_accuracy:
        rec['accuracy'] = accuracy()
    rec['timing'] = timing(args)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_buoyant_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
