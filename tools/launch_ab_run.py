"""Developer helper for same-box A/B of HOST-side changes to the launch path (the kernels' code objects being equal): the cases where launches,
not kernels, set the time, and digests of results to compare two builds bit for bit.  One fresh process per call; the library is the in-tree
build or NNS_LIB_PATH (tools/ab_build.sh).  Prints ONE JSON line.

    [NNS_LIB_PATH=...] python tools/launch_ab_run.py time [--steps 400]
        wall-clock microseconds per step (host loop + device, one synchronisation after the loop; warmed with the same number of steps):
        the eager PeriodicSolver.step loop at 64^2 x 1 and 256^2 x 64, the chorin_fd explicit cavity step at 16^2 (simulate_device, no graph)
    [NNS_LIB_PATH=...] python tools/launch_ab_run.py digest
        sha256 of PeriodicSolver.simulate frames (128^2 x 2, 6 steps, eager) and of the six outputs of ops.residual_both (256^2 x 4)"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'neural-navier-stokes_amd'), os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import pspec_oracle as O  # noqa: E402
from nns import _lib, ops  # noqa: E402
from nns.periodic import PeriodicSolver  # noqa: E402

dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device='cuda')


def wall_us(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / steps * 1e6, 2)


def pspec_loop(n, B, steps):
    s = PeriodicSolver(n, n, 1e-3, 1.0, 1e-3)
    u0, v0 = O.random_ic(B, n, n, 8, seed=n + B, umax=1.0)
    st = s.init(dev(u0), dev(v0))

    def loop():
        for _ in range(steps):
            s.step(st)
    return wall_us(loop, steps)


def cavity(m, steps):
    from nns.chorin_fd import NavierStokesSystem
    from oracle.boundary import cavity_bcs
    dx = dy = 2. / (m - 1)
    u_bc, v_bc, p_bc = cavity_bcs(dx, dy)
    z = np.zeros((m, m))
    s = NavierStokesSystem(z.copy(), z.copy(), z.copy(), u_bc, v_bc, p_bc, nt=steps, nit=50, nx=m, ny=m, dt=1e-3, rho=1, nu=0.1, beta=1.25,
                           method='explicit')
    return wall_us(lambda: s.simulate_device(use_graph=False), steps)


def digest():
    from nns.synthetic import residual_inputs
    sha = lambda ts: hashlib.sha256(b''.join(t.detach().cpu().numpy().tobytes() for t in ts)).hexdigest()
    s = PeriodicSolver(128, 128, 1e-3, 1.0, 1e-3)
    u0, v0 = O.random_ic(2, 128, 128, 8, seed=7, umax=1.0)
    frames = s.simulate(dev(u0), dev(v0), 6, save_every=2, use_graph=False)
    f = [torch.as_tensor(a, device='cuda') for a in residual_inputs(4, 256, dt=1e-3, nu=2 * np.pi / 1000, rho=1.0)]
    fd, sp = ops.residual_both(*f, 1e-3, 2 * np.pi, 2 * np.pi, 1.0, 2 * np.pi / 1000)
    return dict(simulate_frames=sha([torch.as_tensor(a) for a in frames]), residual_both=sha(list(fd) + list(sp)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['time', 'digest'])
    ap.add_argument('--steps', type=int, default=400)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rec = dict(lib=os.path.relpath(_lib.LIB_PATH, ROOT))
    if args.what == 'digest':
        rec.update(digest())
    else:
        rec.update(steps=args.steps, pspec_64x1_us=pspec_loop(64, 1, args.steps), pspec_256x64_us=pspec_loop(256, 64, args.steps),
                   cavity_16_us=cavity(16, args.steps))
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
