"""Measures the Lagrangian tracers of the periodic spectral solver (nns.periodic.PeriodicSolver.init_particles / sample / advect:
nns_spec_ns_particle_* of csrc/pspec_particles.hip).  Writes ONE JSON record to OUTDIR/pspec_particles_run.json and prints it.

    python tools/pspec_particles_run.py OUTDIR [--steps 8] [--reps 7] [--commit ID] [--parent-lib PATH] [--no-accuracy] [--no-timing]

Accuracy (tests/pspec_particles_cases.py, the figures tests/test_gpu_pspec_particles.py bounds): the coefficient images and the samples of u, v,
w, theta at both shapes and orders, and the positions after ``advect`` on the four solvers under both schemes, against the float64
restatement; MEASURED of the cases module is the worst of each kind and its bounds are 4x those.
Timing: at 256^2 x 64 with 65 536 particles per grid and at 1024^2 x 8 with 1 048 576 (|m| <= 8 flow, Kolmogorov force k = 4, drag 0.1,
particles uniform over the box) these take turns within every repetition: ``advect`` ('rk4') with order 4 and with order 6, ``step`` alone,
``step`` of another build of the library (--parent-lib: the parent commit's; twice, with this build's turn between them, so that the ratio of
its two turns is the noise the A/B ratio is read against; also whether both builds give the same bits), the coefficient builds of those steps
alone, the stage launches alone, one ``sample`` of (u, v), and what a user composed before: the same RK4 over pairs of steps with ``fields()``
at every step boundary and the velocity read by torch index arithmetic (bilinear, float32 positions).  A timing is device events around the
work, reported per flow step as the median over the repetitions with the spread (max - min) / median; ratios are medians of the
per-repetition ratios.  One coefficient layout was built (an image per field); the interleaved (u, v) image was not tried."""
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
from nns import _lib, ops  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402
from pspec_adjoint_run import event_ms, stats, ratio, dev  # noqa: E402

CASES = [(256, 64, 65536), (1024, 8, 1048576)]
DT, NU, DRAG = 1e-3, 1e-3, 0.1


def parent_step(path):
    """The forced step of another build of the library, under the argument list of include/nns.h."""
    L = ctypes.CDLL(path)
    I, D, P, Z = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    L.nns_spec_ns_step_forced_f32.argtypes = [P] * 3 + [I, P, Z] + [I] * 3 + [D] * 5 + [I, P]

    def step(s, st, n):
        rc = L.nns_spec_ns_step_forced_f32(st.what.data_ptr(), st.mean.data_ptr(), s.ghat.data_ptr(), s.ghat.shape[0], st.work.data_ptr(),
                                           st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, n,
                                           torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('the library refused the step: %d' % rc)
    return step


def composed(s, state, pos, nsteps, out):
    """RK4 over pairs of steps as a user composed it before: fields() at every step boundary, bilinear reads by torch index arithmetic on
    float32 positions [B, P, 2]."""
    nx, ny, dt = s.nx, s.ny, s.dt
    scale = torch.tensor([nx / s.Lx, ny / s.Ly], dtype=torch.float32, device=pos.device)
    bidx = torch.arange(state.batch, device=pos.device)[:, None]

    def read(u, v, x):
        g = x * scale
        f = torch.floor(g)
        t = g - f
        i, j = f[..., 0].long() % nx, f[..., 1].long() % ny
        i1, j1 = (i + 1) % nx, (j + 1) % ny
        tx, ty = t[..., 0], t[..., 1]
        lerp = lambda a: ((1 - tx) * ((1 - ty) * a[bidx, i, j] + ty * a[bidx, i, j1]) + tx * ((1 - ty) * a[bidx, i1, j] + ty * a[bidx, i1, j1]))
        return torch.stack([lerp(u), lerp(v)], dim=-1)
    u, v, _ = s.fields(state, out=out[0])
    for _ in range(nsteps // 2):
        k1 = read(u, v, pos)
        s.step(state, 1)
        u1, v1, _ = s.fields(state, out=out[1])
        k2 = read(u1, v1, pos + dt * k1)
        k3 = read(u1, v1, pos + dt * k2)
        s.step(state, 1)
        u, v, _ = s.fields(state, out=out[0])
        k4 = read(u, v, pos + 2 * dt * k3)
        pos = pos + (dt / 3) * (k1 + 2 * k2 + 2 * k3 + k4)
    return pos


def timing(args):
    out = []
    steps = args.steps
    parent = parent_step(args.parent_lib) if args.parent_lib else None
    this = parent_step(_lib.LIB_PATH)
    for n, B, P in CASES:
        s = PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG).kolmogorov_forcing(4, 1.0)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        st0 = s.init(dev(u0), dev(v0))
        s.step(st0, 20)                                                   # a developed state
        rng = np.random.default_rng(n)
        xy = torch.as_tensor(rng.uniform(0.0, 2 * np.pi, (B, P, 2)), device='cuda')
        parts = {order: s.init_particles(xy[..., 0], xy[..., 1], order=order) for order in (4, 6)}
        pos32 = xy.float()
        frames = [tuple(torch.empty((B, n, n), dtype=torch.float32, device='cuda') for _ in range(3)) for _ in range(2)]
        st = st0.clone()
        p4 = parts[4]

        def restore():
            st.what.copy_(st0.what)
            for order in parts:
                parts[order].pos.copy_(xy)

        def builds():
            for k in range(steps):
                s._coefficients(st, 3, 4, p4._coef[k % 2], p4._work)

        def stages(order):
            p = parts[order]

            def run():
                for k in range(steps):
                    ops.spec_ns_particle_stage_(p._coef[0], p.pos, p.pos, p._stage, p._acc, s.dt, 1.0, 0.0, True, False, order, s.Lx, s.Ly)
                    ops.spec_ns_particle_stage_(p._coef[0], p.pos, p._stage, p._stage, p._acc, s.dt, 2.0, 0.0, False, False, order, s.Lx, s.Ly)
            return run
        variants = [('advect_order4', lambda: s.advect(st, parts[4], steps)), ('advect_order6', lambda: s.advect(st, parts[6], steps)),
                    ('step', lambda: s.step(st, steps)), ('coefficient_builds', builds), ('stages_order4', stages(4)), ('stages_order6', stages(6)),
                    ('sample_uv_order4_one_call', lambda: s.sample(st, parts[4])), ('sample_uv_order6_one_call', lambda: s.sample(st, parts[6])),
                    ('composed_fields_torch_bilinear', lambda: composed(s, st, pos32, steps, frames))]
        case = dict(nx=n, ny=n, batch=B, particles_per_grid=P)
        if parent:
            restore()
            this(s, st, steps)
            mine = st.what.clone()
            restore()
            parent(s, st, steps)
            case['step_bitwise_parent_lib'] = bool(torch.equal(mine, st.what))
            variants += [('step_parent_lib', lambda: parent(s, st, steps)), ('step_direct', lambda: this(s, st, steps)),
                         ('step_parent_lib_again', lambda: parent(s, st, steps))]
        restore()
        s.advect(st, parts[4], steps)
        after = st.what.clone()
        restore()
        s.step(st, steps)
        case['advect_state_bitwise_step'] = bool(torch.equal(after, st.what))
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
            case[name] = stats(ts[name], 1 if 'one_call' in name else steps)
        for order in (4, 6):
            case['advect_order%d_over_step' % order] = ratio(ts['advect_order%d' % order], ts['step'])
            case['composed_over_advect_order%d' % order] = ratio(ts['composed_fields_torch_bilinear'], ts['advect_order%d' % order])
        case['coefficient_builds_over_step'] = ratio(ts['coefficient_builds'], ts['step'])
        case['stages_order4_over_step'] = ratio(ts['stages_order4'], ts['step'])
        case['stages_order6_over_stages_order4'] = ratio(ts['stages_order6'], ts['stages_order4'])
        if parent:
            case['step_over_parent_lib'] = ratio(ts['step_direct'], ts['step_parent_lib'])
            case['step_parent_lib_again_over_parent_lib'] = ratio(ts['step_parent_lib_again'], ts['step_parent_lib'])
        out.append(case)
        print(json.dumps(case), flush=True)
        del st, st0, parts, frames, xy, pos32, p4
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_particles_cases as PC
    import pspec_particles_oracle as PO
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    rows, worst = [], dict(coef=0.0, sample=0.0, advect=0.0)

    def setup(kind, shape, order):
        d = PC.inputs(shape)
        s = PC.solver(kind, shape)
        state = s.init(dev(d['u0']), dev(d['v0']), dev(d['theta0']) if kind == 'buoyant' else None)
        pos = PC.positions(shape)
        return s, state, s.init_particles(pos[..., 0], pos[..., 1], order=order, device='cuda')
    for shape in PC.SHAPES:
        for order in PC.ORDERS:
            s, state, p = setup('buoyant', shape, order)
            coef_ref, val_ref = PC.oracle_read(shape, order)
            coef, vals = s.particle_coefficients(state, PC.FIELDS, order), s.sample(state, p, PC.FIELDS)
            for k, f in enumerate(PC.FIELDS):
                ec, es = PC.rel_max(host(coef[k]), coef_ref[f]), PC.rel_max(host(vals[..., k]), val_ref[f])
                worst['coef'], worst['sample'] = max(worst['coef'], ec), max(worst['sample'], es)
                rows.append(dict(shape=PC.shape_id(shape), order=order, field=f, coef=float('%.3e' % ec), sample=float('%.3e' % es)))
    S, w, mean, _ = PC.start('plain', PC.WIDE)
    pos = PC.positions(PC.WIDE)
    s, state, p = setup('plain', PC.WIDE, 4)
    got, ref = host(s.sample(state, p)), PO.Tracers(S, 4).sample(w, mean, pos)
    for k, f in enumerate(('u', 'v')):
        es = PC.rel_max(got[..., k], ref[..., k])
        worst['sample'] = max(worst['sample'], es)
        rows.append(dict(shape=PC.shape_id(PC.WIDE), order=4, field=f, sample=float('%.3e' % es)))
    runs = [(kind, PC.SQUARE, sc, n, order) for kind in PC.KINDS for sc, n in PC.SCHEMES for order in (PC.ORDERS if kind == 'plain' else (4,))]
    runs.append(('plain', PC.OBLONG, 'rk4', 4, 6))
    for kind, shape, sc, n, order in runs:
        s, state, p = setup(kind, shape, order)
        s.advect(state, p, n, sc)
        e = PC.displacement_error(host(p.pos), PC.oracle_advect(kind, shape, sc, n, order), PC.positions(shape))
        worst['advect'] = max(worst['advect'], e)
        rows.append(dict(kind=kind, shape=PC.shape_id(shape), scheme=sc, steps=n, order=order, advect=float('%.3e' % e)))
    for r in rows:
        print(json.dumps(r), flush=True)
    return dict(rows=rows, worst={k: float('%.3e' % v) for k, v in worst.items()},
                bounds=dict(coef=PC.COEF_BOUND, sample=PC.SAMPLE_BOUND, advect=PC.ADVECT_BOUND))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--steps', type=int, default=8, help='flow steps per timing (even)')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's) for the same-process comparison")
    ap.add_argument('--no-accuracy', action='store_true')
    ap.add_argument('--no-timing', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, steps=args.steps, reps=args.reps, parent_lib=bool(args.parent_lib))
    if not args.no_accuracy:
        rec['accuracy'] = accuracy()
    if not args.no_timing:
        rec['timing'] = timing(args)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_particles_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
