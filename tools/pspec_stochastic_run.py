"""Measures the white-in-time stochastic forcing of the periodic spectral solver (nns.periodic.PeriodicSolver.ring_forcing /
set_stochastic_forcing: nns_spec_ns_step_stochastic_f32 of csrc/pspec_kernels.hip).  Writes ONE JSON record to OUTDIR/pspec_stochastic_run.json
and prints it.

    python tools/pspec_stochastic_run.py OUTDIR [--steps 100] [--reps 7] [--commit ID] [--parent-lib PATH] [--no-accuracy]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow, Kolmogorov force k = 4, drag 0.1, ring force on 4 <= k_s <= 6) the stochastic,
steady-forced and unforced steps take turns within every repetition, each from the same saved state (restored outside the timed window); with
--parent-lib also the steady-forced and unforced steps of another build of the library (the parent commit's), loaded into the same process and
called on the same buffers, and whether they give the same bits.  A timing is device events around one call of `steps` steps, reported per step
as the median over the repetitions with the spread (max - min) / median; the ratios are medians of the per-repetition ratios.
Accuracy (tests/pspec_stochastic_cases.py, the figures tests/test_gpu_pspec_stochastic.py bounds): the kick of one step from rest against the
oracle's Philox on every forced mode (worst error over the tolerance, and the moments of the samples), and the trajectories after 12 steps
against the float64 restatement."""
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
RING, RATE, SEED = (4.0, 6.0), 0.1, 2024


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
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


def parent_steps(path):
    """The steady-forced and unforced steps of another build of the library, through its own ctypes handle."""
    L = ctypes.CDLL(path)
    I, D, P = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    L.nns_spec_ns_step_forced_f32.argtypes = [P] * 3 + [I, P, ctypes.c_size_t] + [I] * 3 + [D] * 5 + [I, P]
    L.nns_spec_ns_step_f32.argtypes = [P] * 3 + [ctypes.c_size_t] + [I] * 3 + [D] * 4 + [I, P]

    def forced(s, st, nsteps):
        rc = L.nns_spec_ns_step_forced_f32(st.what.data_ptr(), st.mean.data_ptr(), s.ghat.data_ptr(), int(s.ghat.shape[0]), st.work.data_ptr(),
                                           st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, nsteps,
                                           torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('the parent library refused the forced step: %d' % rc)

    def unforced(s, st, nsteps):
        rc = L.nns_spec_ns_step_f32(st.what.data_ptr(), st.mean.data_ptr(), st.work.data_ptr(), st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly,
                                    s.dt, s.nu, nsteps, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('the parent library refused the step: %d' % rc)
    return forced, unforced


def timing(args):
    out = []
    parent = parent_steps(args.parent_lib) if args.parent_lib else None
    for n, B in CASES:
        forced = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1).kolmogorov_forcing(4, 1.0)
        stoch = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3, drag=0.1).kolmogorov_forcing(4, 1.0).ring_forcing(RATE, RING[0], RING[1], seed=SEED)
        plain = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        st = stoch.init(dev(u0), dev(v0))
        stoch.step(st, 20)                                                # a developed state
        saved = st.clone()

        def restore():
            st.what.copy_(saved.what), st.clock.copy_(saved.clock)

        variants = [('stochastic', lambda: stoch.step(st, args.steps)), ('forced', lambda: forced.step(st, args.steps)),
                    ('unforced', lambda: plain.step(st, args.steps))]
        case = dict(nx=n, ny=n, batch=B, forced_stored_modes=int(np.count_nonzero(stoch.stoch_amp)))
        if parent:
            variants += [('forced_parent_lib', lambda: parent[0](forced, st, args.steps)), ('unforced_parent_lib', lambda: parent[1](plain, st, args.steps))]
            for name, s, k in (('forced', forced, 0), ('unforced', plain, 1)):        # the same instructions: the same bits
                restore()
                s.step(st, 3)
                mine = st.what.clone()
                restore()
                parent[k](s, st, 3)
                case[name + '_bitwise_parent_lib'] = bool(torch.equal(mine, st.what))
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
        case['stochastic_over_forced'] = ratio(ts['stochastic'], ts['forced'])
        case['forced_over_unforced'] = ratio(ts['forced'], ts['unforced'])
        if parent:
            case['forced_over_parent_lib'] = ratio(ts['forced'], ts['forced_parent_lib'])
            case['unforced_over_parent_lib'] = ratio(ts['unforced'], ts['unforced_parent_lib'])
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, saved
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_buoyant_cases as BC
    import pspec_cases as C
    import pspec_forced_cases as FC
    import pspec_scalar_cases as SC
    import pspec_stochastic_cases as XC
    host = lambda t: t.cpu().numpy().astype(np.float64)
    cplx = lambda t: host(t)[..., 0] + 1j * host(t)[..., 1]
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
    r3 = lambda x: float('%.3e' % x)
    kicks, traj = [], []
    for case in XC.KICKS:
        nx, ny, B, Lx, Ly = case
        s = PeriodicSolver(nx, ny, XC.KICK_DT, C.RHO, 0.0, Lx=Lx, Ly=Ly).ring_forcing(XC.KICK_RATE, *XC.kick_ring(*case), seed=XC.SEED)
        z = torch.zeros(B, nx, ny, device='cuda')
        st = s.step(s.init(z, z), 1)
        mask, xi = XC.kick_samples(case)
        a = s.stoch_amp.astype(np.float64)[mask][None] * np.sqrt(XC.KICK_DT)
        got = cplx(st.what[:, torch.as_tensor(mask, device='cuda')])
        m2, m1, bound = XC.moments(got / a)
        kicks.append(dict(nx=nx, ny=ny, batch=B, forced_stored_modes=int(mask.sum()),
                          worst_error_over_tolerance=r3((np.abs(got - a * xi) / (XC.KICK_TOL * a * np.maximum(1.0, np.abs(xi)))).max()),
                          mean_abs2_minus_1=r3(m2), abs_mean=r3(m1), moment_bound=r3(bound)))
        print(json.dumps(kicks[-1]), flush=True)
    for kind, case in [('flow', c) for c in XC.TRAJ] + [('scalar', XC.SCALAR_CASE), ('buoyant', XC.BUOYANT_CASE)]:
        nx, ny, B, Lx, Ly, _ = case
        S, X, ins, w, t, mean, rate, ratio_ = XC.reference(kind, case)
        kw = {} if kind == 'flow' else dict(kappa=SC.KAPPA, scalar_gradient=SC.GRAD)
        if kind == 'buoyant':
            kw['buoyancy'] = BC.BUOY
        s = PeriodicSolver(nx, ny, S.dt, C.RHO, C.NU, Lx=Lx, Ly=Ly, drag=FC.DRAG, **kw).kolmogorov_forcing(FC.KF, FC.AMP)
        s.ring_forcing(rate, *XC.traj_ring(nx, ny, Lx, Ly), seed=XC.SEED)
        st = s.step(s.init(*[dev(a) for a in ins]), XC.NSTEPS)
        u, v, p = (host(f) for f in s.fields(st))
        ru, rv, rp = S.fields(w, mean, t) if kind == 'buoyant' else S.fields(w, mean)
        r = dict(kind=kind, nx=nx, ny=ny, batch=B, steps=XC.NSTEPS, rate=r3(rate), injected_over_initial_energy=round(ratio_, 3),
                 what=r3(rel(cplx(st.what), S.compact(w))), u=r3(rel(u, ru)), v=r3(rel(v, rv)), p=r3(rel(p, rp)))
        if t is not None:
            r['that_fluct'] = r3(rel(S.compact(S.fluctuation(S.expand(cplx(st.that)))), S.compact(S.fluctuation(t))))
        traj.append(r)
        print(json.dumps(r), flush=True)
    return dict(kick=kicks, trajectories=traj)


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
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps, ring=list(RING), rate=RATE)
    if not args.no_accuracy:
        rec['accuracy'] = accuracy()
    rec['timing'] = timing(args)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_stochastic_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
