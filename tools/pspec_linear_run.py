"""Measures the general linear operator of the periodic spectral solver (nns.periodic.PeriodicSolver with hyperviscosity, hypofriction and beta:
nns_spec_ns_step_linear_f32 and nns_spec_ns_linear_spectrum_f32 of csrc/pspec_kernels.hip).  Writes ONE JSON record to
OUTDIR/pspec_linear_run.json and prints it.

    python tools/pspec_linear_run.py OUTDIR [--steps 100] [--reps 7] [--commit ID] [--parent-lib PATH] [--no-accuracy]

Timing: at 256^2 x 64 and 1024^2 x 8 (|m| <= 8 flow, Kolmogorov force k = 4, drag 0.1) the linear step (nu_h, p = 4; mu, q = 1; beta), the
steady-forced step, the stochastic step (ring 4 <= k_s <= 6), the linear step with that ring force and the scalar step take turns within every
repetition, each from the same saved state (restored outside the timed window); with --parent-lib also the steady-forced, scalar and stochastic
steps of another build of the library (the parent commit's), loaded into the same process and called on the same buffers, and whether they give
the same bits.  A timing is device events around one call of `steps` steps, reported per step as the median over the repetitions with the
spread (max - min) / median; the ratios are medians of the per-repetition ratios.  One linear_spectrum call is timed the same way (100 calls).
The byte model: the linear step reads 8 bytes per stored mode of ONE grid in each of stages 1-3 (the table is shared by the batch and stays
in L2), against the 8 launches' traffic of the forced step, 2 x 8 bytes per mode and grid for W and A in the column pass alone.
Accuracy (tests/pspec_linear_cases.py, the figures tests/test_gpu_pspec_linear.py bounds): the trajectories after 12 steps against the float64
restatement, the Rossby wave after 200 steps against the analytic solution, and the stiff step."""
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
DT, NU, DRAG, KAPPA, GRAD = 1e-3, 1e-3, 0.1, 2e-3, (0.7, -0.4)


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


def linear_kw(n):
    """Per step: 5 at the band's corner from the hyperviscosity, 0.05 on the gravest mode from the hypofriction, 0.2 rad from beta."""
    K = np.hypot((n - 1) // 3, (n - 1) // 3)
    return dict(hyperviscosity=(5.0 / (DT * K ** 8), 4), hypofriction=(0.05 / DT, 1), beta=0.2 / DT)


def parent_steps(path):
    """The steady-forced, scalar and stochastic steps of another build of the library, through its own ctypes handle."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_forced_f32.argtypes = [P] * 3 + [I, P, Z] + [I] * 3 + [D] * 5 + [I, P]
    L.nns_spec_ns_step_scalar_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 8 + [I, P]
    L.nns_spec_ns_step_stochastic_f32.argtypes = [P] * 4 + [I, P, Z] + [I] * 3 + [D] * 10 + [P, ctypes.c_uint64, P, P, I, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def check(rc):
        if rc != 0:
            raise RuntimeError('the parent library refused the step: %d' % rc)

    def forced(s, st, n):
        check(L.nns_spec_ns_step_forced_f32(st.what.data_ptr(), st.mean.data_ptr(), s.ghat.data_ptr(), int(s.ghat.shape[0]), st.work.data_ptr(),
                                            st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, n, stream()))

    def scalar(s, st, n):
        check(L.nns_spec_ns_step_scalar_f32(st.what.data_ptr(), st.that.data_ptr(), st.mean.data_ptr(), s.ghat.data_ptr(), int(s.ghat.shape[0]),
                                            st.work.data_ptr(), st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, s.kappa,
                                            s.scalar_gradient[0], s.scalar_gradient[1], n, stream()))

    def stochastic(s, st, n):
        amp, clock, ids = s._noise_of(st)
        check(L.nns_spec_ns_step_stochastic_f32(st.what.data_ptr(), None, st.mean.data_ptr(), s.ghat.data_ptr(), int(s.ghat.shape[0]),
                                                st.work.data_ptr(), st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, 0.0, 0.0,
                                                0.0, 0.0, 0.0, amp.data_ptr(), s.stoch_seed, clock.data_ptr(), ids.data_ptr(), n, stream()))
    return dict(forced=forced, scalar=scalar, stochastic=stochastic)


def timing(args):
    out = []
    parent = parent_steps(args.parent_lib) if args.parent_lib else None
    for n, B in CASES:
        mk = lambda **kw: PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG, **kw).kolmogorov_forcing(4, 1.0)
        solvers = dict(forced=mk(), linear=mk(**linear_kw(n)), stochastic=mk().ring_forcing(RATE, RING[0], RING[1], seed=SEED),
                       linear_stochastic=mk(**linear_kw(n)).ring_forcing(RATE, RING[0], RING[1], seed=SEED),
                       scalar=mk(kappa=KAPPA, scalar_gradient=GRAD))
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        th0 = O.random_ic(B, n, n, 8, seed=n + B + 1, umax=1.0)[0]
        st = solvers['linear_stochastic'].init(dev(u0), dev(v0))
        sts = solvers['scalar'].init(dev(u0), dev(v0), dev(th0))
        solvers['linear_stochastic'].step(st, 20)                         # a developed state
        solvers['scalar'].step(sts, 20)
        saved, saveds = st.clone(), sts.clone()

        def restore():
            st.what.copy_(saved.what), st.clock.copy_(saved.clock), sts.what.copy_(saveds.what), sts.that.copy_(saveds.that)

        state = lambda name: sts if name == 'scalar' else st
        variants = [(name, (lambda s=s, name=name: s.step(state(name), args.steps))) for name, s in solvers.items()]
        case = dict(nx=n, ny=n, batch=B)
        if parent:
            for name in ('forced', 'scalar', 'stochastic'):
                variants.append((name + '_parent_lib', (lambda name=name: parent[name](solvers[name], state(name), args.steps))))
                restore()
                solvers[name].step(state(name), 3)
                mine = state(name).what.clone()
                restore()
                parent[name](solvers[name], state(name), 3)
                case[name + '_bitwise_parent_lib'] = bool(torch.equal(mine, state(name).what))
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
        case['linear_over_forced'] = ratio(ts['linear'], ts['forced'])
        case['stochastic_over_forced'] = ratio(ts['stochastic'], ts['forced'])
        case['linear_stochastic_over_stochastic'] = ratio(ts['linear_stochastic'], ts['stochastic'])
        if parent:
            for name in ('forced', 'scalar', 'stochastic'):
                case[name + '_over_parent_lib'] = ratio(ts[name], ts[name + '_parent_lib'])
        restore()
        lin = solvers['linear']
        lin.linear_spectrum(st)
        torch.cuda.synchronize()
        case['linear_spectrum_call'] = stats([event_ms(lambda: [lin.linear_spectrum(st) for _ in range(100)]) for _ in range(args.reps)], 100)
        my1 = lin.my1
        case['byte_model'] = dict(table_bytes=8 * my1 * n, table_reads_per_step=3,
                                  column_pass_state_bytes_per_step=int(8 * B * my1 * n * (2 + 3 + 3 + 3 + 2)),
                                  table_over_state=round(3 * 8 * my1 * n / float(8 * B * my1 * n * 13), 5))
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, sts, saved, saveds
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_buoyant_cases as BC
    import pspec_cases as C
    import pspec_linear_cases as LC
    import pspec_linear_oracle as LO
    import pspec_stochastic_cases as XC
    host = lambda t: t.cpu().numpy().astype(np.float64)
    cplx = lambda t: host(t)[..., 0] + 1j * host(t)[..., 1]
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))
    r3 = lambda x: float('%.3e' % x)
    traj = []
    for kind, case in [('flow', c) for c in LC.CASES] + [('scalar', LC.SCALAR_CASE), ('buoyant', LC.BUOYANT_CASE), ('stochastic', LC.CASES[0])]:
        nx, ny, B, Lx, Ly, _ = case
        S, ins, w, t, mean, extra = LC.reference(kind, case)
        stoch = None if extra is None else (extra[0],) + tuple(XC.traj_ring(nx, ny, Lx, Ly))
        s = LC.solver(case, S.dt, 'flow' if kind == 'stochastic' else kind, stochastic=stoch)
        st = s.step(s.init(*[dev(a) for a in ins]), LC.NSTEPS)
        u, v, p = (host(f) for f in s.fields(st))
        ru, rv, rp = S.fields(w, mean, t) if kind == 'buoyant' else S.fields(w, mean)
        r = dict(kind=kind, nx=nx, ny=ny, batch=B, steps=LC.NSTEPS, what=r3(rel(cplx(st.what), S.compact(w))), u=r3(rel(u, ru)), v=r3(rel(v, rv)),
                 p=r3(rel(p, rp)))
        if t is not None:
            r['that_fluct'] = r3(rel(S.compact(S.fluctuation(S.expand(cplx(st.that)))), S.compact(S.fluctuation(t))))
        traj.append(r)
        print(json.dumps(r), flush=True)
    nx, ny, Lx, Ly, m, U, dt = LC.WAVE
    s = PeriodicSolver(nx, ny, dt, C.RHO, LC.WAVE_NU, Lx=Lx, Ly=Ly, drag=LC.WAVE_DRAG, hyperviscosity=LC.WAVE_HYPER, hypofriction=LC.WAVE_HYPO,
                       beta=LC.WAVE_BETA)
    u0, v0 = LO.rossby_wave(nx, ny, 0.0, m, LC.WAVE_BETA, LC.wave_damping(), U, Lx, Ly)[:2]
    st = s.step(s.init(dev(u0), dev(v0)), LC.WAVE_STEPS)
    ru, rv, rw, A, om = LO.rossby_wave(nx, ny, LC.WAVE_STEPS * dt, m, LC.WAVE_BETA, LC.wave_damping(), U, Lx, Ly)
    S = LO.LinearScheme(nx, ny, dt, C.RHO, LC.WAVE_NU, Lx, Ly)
    u, v, p = [host(f)[0] for f in s.fields(st)]
    wave = dict(nx=nx, ny=ny, m=list(m), steps=LC.WAVE_STEPS, omega_t=round(om * LC.WAVE_STEPS * dt, 4), amplitude=round(A, 4),
                w=r3(np.abs(S.irfft2(S.expand(cplx(st.what)))[0] - rw).max() / A), uv=r3(max(np.abs(u - ru).max(), np.abs(v - rv).max()) / A),
                bound=LC.WAVE_BOUND)
    print(json.dumps(wave), flush=True)
    case = LC.CASES[0]
    nx, ny, B, Lx, Ly, _ = case
    u0, v0, dt = C.full_band_input(*case)
    pr = LC.params(nx, ny, Lx, Ly, dt, hyper_per_step=LC.STIFF_PER_STEP)
    S = LC.scheme(nx, ny, dt, Lx, Ly, hyper=pr['hyper'])
    w0, mean = S.init(u0, v0)
    w = S.step(w0, mean, 1)
    s = LC.solver(case, dt, hyperviscosity=pr['hyper'])
    st = s.step(s.init(dev(u0), dev(v0)), 1)
    fu, fv, fp = (host(f) for f in s.fields(st))
    ru, rv, rp = S.fields(w, mean)
    stiff = dict(nx=nx, ny=ny, per_step=LC.STIFF_PER_STEP, what=r3(rel(cplx(st.what), S.compact(w))), u=r3(rel(fu, ru)), v=r3(rel(fv, rv)),
                 p=r3(rel(fp, rp)))
    print(json.dumps(stiff), flush=True)
    return dict(trajectories=traj, rossby_wave=wave, stiff_step=stiff, bounds=dict(what=C.BOUND_W, uv=C.BOUND_UV, p=C.BOUND_P, p_buoyant=BC.BOUND_P))


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
    with open(os.path.join(args.outdir, 'pspec_linear_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
