"""Measures the reverse mode of particle sampling of the periodic spectral solver (nns.periodic.PeriodicSolver.observe / spread /
sample_gradient / particle_cells: nns_spec_ns_particle_cells_i32, _spread_f32, _sample_grad_f32, _coefs_adjoint_f32 of
csrc/pspec_particles.hip).  Writes ONE JSON record to OUTDIR/pspec_particles_adjoint_run.json and prints it.

    python tools/pspec_particles_adjoint_run.py OUTDIR [--reps 7] [--commit ID] [--parent-lib PATH] [--no-accuracy] [--no-timing]

Accuracy (tests/pspec_particles_adjoint_cases.py, the figures tests/test_gpu_pspec_particles_adjoint.py bounds): every quantity of that file's
checks on its own cases against the float64 restatement, the worst of each; MEASURED of the cases module holds them and its bounds are 4x.
Timing: at 256^2 x 64 and 1024^2 x 8 with one particle per node (a fixed offset in every cell), orders 4 and 6, these take turns within
every repetition: ``sample`` of (u, v) (coefficient build and gather) and the gather alone; the backward into w in its parts -- the cells
launch with the stable sort and the searchsorted, the spread (staging and node launches), the coefficient transpose (2 transforms and a
pointwise launch) -- and whole, as the backward of ``observe``; ``sample_gradient``; and the rival a user composed before: ``fields()``,
bilinear reads by torch index arithmetic and torch autograd back to the (u, v) images, whose scatter is atomic and does not repeat
bitwise.  Then the spread and its sort on a clustered set: the same number of particles in 1 % of the cells, where the node pass's
divergent slot loops show.  The split of the spread into its two launches is read from torch.profiler's kernel times in one extra call
per case (absent where the profiler gives none).  With --parent-lib, ``step``, the coefficient build with the gather, and one Runge-Kutta
stage (what ``advect`` is made of) of that build of the library and of this one: whether the bits agree, and the times A / B / A in the same
process, so that the ratio of the parent's two turns is the noise the A / B ratio is read against.  A timing is device events around the
work: the median over the repetitions with the spread (max - min) / median; ratios are medians of the per-repetition ratios."""
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

CASES = [(256, 64), (1024, 8)]
DT, NU, DRAG = 1e-3, 1e-3, 0.1


def library(path):
    """(step, read, stage) of a build of the library under the argument lists of include/nns.h: the forced step, the coefficient build of
    (u, v) with the gather, and the first Runge-Kutta stage."""
    L = ctypes.CDLL(path)
    I, D, P, Z, G = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_long
    L.nns_spec_ns_step_forced_f32.argtypes = [P] * 3 + [I, P, Z] + [I] * 3 + [D] * 5 + [I, P]
    L.nns_spec_ns_particle_coefs_f32.argtypes = [P] * 4 + [I, I, P, Z] + [I] * 3 + [D, D, P]
    L.nns_spec_ns_particle_sample_f32.argtypes = [P] * 3 + [I] * 3 + [G, I, I, D, D, P]
    L.nns_spec_ns_particle_stage_f32.argtypes = [P] * 5 + [D] * 3 + [I] * 4 + [G, I, I, D, D, P]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def ok(rc):
        if rc != 0:
            raise RuntimeError('the library at %s refused a call: %d' % (path, rc))

    def step(s, st, n):
        ok(L.nns_spec_ns_step_forced_f32(st.what.data_ptr(), st.mean.data_ptr(), s.ghat.data_ptr(), s.ghat.shape[0], st.work.data_ptr(),
                                         st.work.numel(), st.batch, s.nx, s.ny, s.Lx, s.Ly, s.dt, s.nu, s.drag, n, stream()))

    def read(s, st, p, out):
        c, w = p._coef[0], p._work
        ok(L.nns_spec_ns_particle_coefs_f32(st.what.data_ptr(), None, st.mean.data_ptr(), c.data_ptr(), 3, p.order, w.data_ptr(), w.numel(),
                                            st.batch, s.nx, s.ny, s.Lx, s.Ly, stream()))
        ok(L.nns_spec_ns_particle_sample_f32(c.data_ptr(), p.pos.data_ptr(), out.data_ptr(), 2, p.order, st.batch, p.count, s.nx, s.ny, s.Lx,
                                             s.Ly, stream()))

    def stage(s, st, p):
        ok(L.nns_spec_ns_particle_stage_f32(p._coef[0].data_ptr(), p.pos.data_ptr(), p.pos.data_ptr(), p._stage.data_ptr(), p._acc.data_ptr(),
                                            s.dt, 1.0, 0.0, 1, 0, p.order, st.batch, p.count, s.nx, s.ny, s.Lx, s.Ly, stream()))
    return step, read, stage


def bilinear(u, v, pos, scale, bidx, nx, ny):
    g = pos * scale
    f = torch.floor(g)
    t = g - f
    i, j = f[..., 0].long() % nx, f[..., 1].long() % ny
    i1, j1 = (i + 1) % nx, (j + 1) % ny
    tx, ty = t[..., 0], t[..., 1]
    lerp = lambda a: ((1 - tx) * ((1 - ty) * a[bidx, i, j] + ty * a[bidx, i, j1]) + tx * ((1 - ty) * a[bidx, i1, j] + ty * a[bidx, i1, j1]))
    return torch.stack([lerp(u), lerp(v)], dim=-1)


def kernel_split(fn):
    """{kernel name fragment: device ms} of the two spread launches in one call of fn, from torch.profiler; {} where it gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for frag in ('spread_stage', 'spread_node'):
                if frag in e.key:
                    us = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
                    out[frag] = round(out.get(frag, 0.0) + us / 1000.0, 5)
        return out
    except Exception as exc:                                   # a measurement aid only: the record says that the split is absent
        return dict(unmeasured=str(exc)[:200])


def timing(args):
    out = []
    parent = library(args.parent_lib) if args.parent_lib else None
    this = library(_lib.LIB_PATH)
    for n, B in CASES:
        s = PeriodicSolver(n, n, DT, 1.0, NU, drag=DRAG).kolmogorov_forcing(4, 1.0)
        u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
        st = s.init(dev(u0), dev(v0))
        s.step(st, 20)                                                    # a developed state
        st0 = st.clone()
        h = s.Lx / n
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        one = np.stack([(i.ravel() + 0.37) * h, (j.ravel() + 0.61) * h], axis=-1)
        xy = torch.as_tensor(one, device='cuda').expand(B, -1, -1).contiguous()
        P = xy.shape[1]
        rng = np.random.default_rng(n)
        hot = rng.choice(n * n, n * n // 100, replace=False)
        cells = hot[rng.integers(0, len(hot), (B, P))]
        cl = torch.as_tensor((np.stack([cells // n, cells % n], axis=-1) + rng.uniform(0.01, 0.99, (B, P, 2))) * h, device='cuda')
        r = torch.randn((B, P, 2), device='cuda')
        w = s.vorticity(st)
        scale = torch.tensor([n / s.Lx, n / s.Ly], dtype=torch.float32, device='cuda')
        bidx = torch.arange(B, device='cuda')[:, None]
        pos32 = xy.float()
        case = dict(nx=n, ny=n, batch=B, particles_per_grid=P)
        for order in (4, 6):
            p = s.init_particles(xy[..., 0], xy[..., 1], order=order)
            pc = s.init_particles(cl[..., 0], cl[..., 1], order=order)
            coef = s._coefficients(st, 3, order)
            vals = torch.empty((B, P, 2), dtype=torch.float32, device='cuda')
            perm, start = s.particle_cells(p)
            permc, startc = s.particle_cells(pc)
            cbar = torch.empty_like(coef)
            work = torch.empty(ops.spec_ns_particle_spread_workspace(B, P, order), dtype=torch.uint8, device='cuda')
            x, y = xy[..., 0].contiguous(), xy[..., 1].contiguous()

            def whole():
                wl = w.detach().requires_grad_(True)
                torch.sum(s.observe(wl, x, y, mean=st.mean, order=order) * r).backward()

            def rival():
                u, v, _ = s.fields(st)
                u, v = u.requires_grad_(True), v.requires_grad_(True)
                torch.sum(bilinear(u, v, pos32, scale, bidx, n, n) * r).backward()
            spread = lambda pp, pm, sa: ops.spec_ns_particle_spread(r, pp.pos, pm, sa, n, n, order, s.Lx, s.Ly, out=cbar, work=work)
            variants = [('sample', lambda: s.sample(st, p)),
                        ('gather', lambda: ops.spec_ns_particle_sample(coef, p.pos, order, s.Lx, s.Ly, out=vals)),
                        ('cells_sort', lambda: s.particle_cells(p)),
                        ('spread', lambda: spread(p, perm, start)),
                        ('coefs_adjoint', lambda: ops.spec_ns_particle_coefs_adjoint(cbar, 3, order, s.Lx, s.Ly)),
                        ('observe_forward_backward_w', whole),
                        ('sample_gradient', lambda: s.sample_gradient(st, p)),
                        ('torch_fields_bilinear_autograd', rival),
                        ('cells_sort_clustered', lambda: s.particle_cells(pc)),
                        ('spread_clustered', lambda: spread(pc, permc, startc))]
            rec = {}
            if parent:
                bits = {}
                for name, k in (('step', 0), ('read', 1), ('stage', 2)):
                    got = []
                    for lib in (this, parent):
                        st.what.copy_(st0.what)
                        p.pos.copy_(xy)
                        if k == 0:
                            lib[0](s, st, 4)
                            got.append(st.what.clone())
                        elif k == 1:
                            lib[1](s, st, p, vals)
                            got.append(vals.clone())
                        else:
                            lib[2](s, st, p)
                            got.append(torch.cat([p._stage.reshape(-1), p._acc.reshape(-1)]).clone())
                    bits[name] = bool(torch.equal(got[0], got[1]))
                rec['bitwise_parent_lib'] = bits
                st.what.copy_(st0.what)
                for tag, lib in (('parent_lib', parent), ('this_lib', this), ('parent_lib_again', parent)):
                    variants += [('step_' + tag, lambda lib=lib: lib[0](s, st, 4)), ('read_' + tag, lambda lib=lib: lib[1](s, st, p, vals)),
                                 ('stage_' + tag, lambda lib=lib: lib[2](s, st, p))]
            for _, fn in variants:                             # warm-up: every variant once
                fn()
            torch.cuda.synchronize()
            first = spread(p, perm, start).clone()
            rec['spread_repeats_bitwise'] = bool(torch.equal(first, spread(p, perm, start)))
            ts = {name: [] for name, _ in variants}
            for _ in range(args.reps):
                for name, fn in variants:
                    st.what.copy_(st0.what)
                    torch.cuda.synchronize()
                    ts[name].append(event_ms(fn))
            for name, _ in variants:
                rec[name] = stats(ts[name], 4 if name.startswith('step_') else 1)
            for name in ('cells_sort', 'spread', 'coefs_adjoint', 'observe_forward_backward_w', 'sample_gradient', 'spread_clustered',
                         'torch_fields_bilinear_autograd'):
                rec[name + '_over_gather'] = ratio(ts[name], ts['gather'])
            rec['spread_clustered_over_spread'] = ratio(ts['spread_clustered'], ts['spread'])
            rec['rival_over_observe'] = ratio(ts['torch_fields_bilinear_autograd'], ts['observe_forward_backward_w'])
            if parent:
                for k in ('step', 'read', 'stage'):
                    rec[k + '_this_over_parent'] = ratio(ts[k + '_this_lib'], ts[k + '_parent_lib'])
                    rec[k + '_parent_again_over_parent'] = ratio(ts[k + '_parent_lib_again'], ts[k + '_parent_lib'])
            rec['spread_kernels_ms'] = kernel_split(lambda: spread(p, perm, start))
            rec['spread_clustered_kernels_ms'] = kernel_split(lambda: spread(pc, permc, startc))
            # the byte model: a record per particle written by the staging launch; the node launch reads order^2 records per node (one
            # particle per cell) and 2 order^2 table entries; nf + 1 transforms in the transpose
            rec_bytes = (2 * order + 4) * 4
            rec['model'] = dict(record_bytes=rec_bytes, staging_bytes=B * P * (rec_bytes + 16 + 8 + 8),
                                node_pass_bytes=B * n * n * (order * order * (rec_bytes + 8) + 8))
            case['order%d' % order] = rec
            print(json.dumps({('%dx%d order %d' % (n, B, order)): rec}), flush=True)
            del p, pc, coef, vals, perm, start, permc, startc, cbar, work
            torch.cuda.empty_cache()
        out.append(case)
        del st, st0, xy, cl, r, w, pos32
        torch.cuda.empty_cache()
    return out


def accuracy():
    import pspec_particles_adjoint_cases as AC
    import test_gpu_pspec_particles_adjoint as T
    worst, rows = {}, []

    def note(q, e, case):
        worst[q] = max(worst.get(q, 0.0), e)
        rows.append(dict(case=case, quantity=q, rel_l2=float('%.3e' % e)))
    runs = [(shape, order, B, name) for shape in AC.SHAPES for order in AC.ORDERS for B in AC.BATCHES for name in AC.SETS]
    runs.append((AC.WIDE, 6, 1, 'mixed'))
    for shape, order, B, name in runs:
        case = '%s order %d B %d %s' % (AC.shape_id(shape), order, B, name)
        ref = AC.reference(shape, B, name, order)
        s, state, p, r = T.setup(shape, B, name, order)
        got = dict(spread=torch.stack(s.spread(p, r)), sample_gradient=s.sample_gradient(state, p, AC.ALL))
        _, got['wbar'], got['thetabar'], got['xbar'], got['ybar'] = T.observe_gradients(s, shape, B, name, order)
        for q in got:
            note(q + '_wide' if shape == AC.WIDE and q in ('sample_gradient', 'xbar') else q, AC.rel_l2(T.host(got[q]), ref[q]), case)
        if B == 3 and shape != AC.WIDE:
            nx, ny, Lx, Ly = shape
            c = T.dev(np.random.default_rng(AC.SEED + order).standard_normal((4, 3, nx, ny)))
            Sc = T.host(ops.spec_ns_particle_sample(c, p.pos, order, Lx, Ly))
            lhs, rhs = float(np.sum(Sc * T.host(r))), float(np.sum(T.host(c) * T.host(got['spread'])))
            note('identity', abs(lhs - rhs) / (np.linalg.norm(Sc) * np.linalg.norm(T.host(r))), case)
    # ('theta', 'u', 'u') at shared positions, and the chain through evolve: the test's own cases
    shape, order = AC.OBLONG, 4
    w, th = AC.fields(shape, 3)
    pos, cot = AC.positions(shape, 3, 'mixed'), AC.cotangent(shape, 3, 'mixed')[..., :3].astype(np.float64)
    ref = T.AO.observe_gradients(w, th, AC.MEANS, pos[0, :, 0], pos[0, :, 1], ('theta', 'u', 'u'), cot, shape[2], shape[3], order)
    got = T.observe_gradients(AC.solver(shape, kappa=1e-3), shape, 3, 'mixed', order, ('theta', 'u', 'u'), (0, 1, 2), shared=True)[1:]
    for q, g, f in zip(('wbar', 'thetabar', 'xbar', 'ybar'), got, ref):
        note(q, AC.rel_l2(T.host(g), f), '64x128 order 4 theta,u,u shared')
    note('chain', T.chain_error(), '64x64 order 4, 2 steps')
    for r in rows:
        print(json.dumps(r), flush=True)
    return dict(rows=rows, worst={k: float('%.3e' % v) for k, v in worst.items()}, bounds=dict(AC.BOUND))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('outdir')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--parent-lib', default=None, help="another build of libnns_hip.so (the parent commit's) for the same-process comparison")
    ap.add_argument('--no-accuracy', action='store_true')
    ap.add_argument('--no-timing', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(device=torch.cuda.get_device_name(0), commit=args.commit, reps=args.reps, parent_lib=bool(args.parent_lib))
    if not args.no_accuracy:
        rec['accuracy'] = accuracy()
    if not args.no_timing:
        rec['timing'] = timing(args)
    os.makedirs(args.outdir, exist_ok=True)
    with open(os.path.join(args.outdir, 'pspec_particles_adjoint_run.json'), 'w') as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
