#!/usr/bin/env python3
"""Dense output (-pn_output_times interpolate) against matched output times at BASELINE's C3b shape: MLP 4096 x 512 fp32,
dopri5 adaptive, t = linspace(0, 1, T) for T in {2, 11, 101, 1001}, forward + adjoint per solve.  Then the two dense kernels
alone at n = 2^21 fp32 (the state of C3b), with their algorithmic bytes computed from the shapes:
  pn_rk_dense_eval     (nk + 1 + m) * n * 4     (u and the nk stage derivatives read once, m output rows written)
  pn_rk_dense_adjoint  (m + nd + 1) * n * 4     (m cotangent rows read once, nd vectors D_j and G written)

  python3 tools/bench_dense_output.py [--reps 3] [--out profiles/dense_output.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/bench_dense_output.py --reps 1 --only-kernels
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
import torch  # noqa: E402
from pnode_amd import options, petsc_adjoint  # noqa: E402
from pnode_amd._vecops import HipVecOps  # noqa: E402
from problems import MLPFunc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--only-kernels", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def solve_time(mode, T, reps):
    torch.manual_seed(0)
    f = MLPFunc(512, torch.float32).to(dev)
    y0 = (torch.randn(4096, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(dev)
    options.clear()
    options.set_option("pn_output_times", mode)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, f, step_size=0.01, method="dopri5")
    options.clear()
    t = torch.linspace(0, 1, T, device=dev)
    w = torch.full((T, 4096, 512), 1e-3, device=dev)
    times = []
    for r in range(reps + 1):
        y = y0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (ode.odeint_adjoint(y, t) * w).sum().backward()
        torch.cuda.synchronize()
        if r > 0:
            times.append(time.perf_counter() - t0)
    ms = 1e3 * sorted(times)[len(times) // 2]
    return ode.num_steps, ms


if not a.only_kernels:
    say("C3b (MLP 4096x512 fp32, dopri5 adaptive, t = linspace(0, 1, T)), forward + adjoint, median of %d" % a.reps)
    say("%-12s %6s %7s %12s %14s" % ("mode", "T", "steps", "ms/solve", "time-steps/s"))
    base = {}
    for mode in ("match", "interpolate"):
        for T in (2, 11, 101, 1001):
            steps, ms = solve_time(mode, T, a.reps if not (mode == "match" and T == 1001) else 1)
            base.setdefault(mode, ms)
            say("%-12s %6d %7d %12.2f %14.1f   (x%.3f of T = 2)" % (mode, T, steps, ms, 1e3 * steps / ms, ms / base[mode]))

n = 1 << 21
ops = HipVecOps(dev, torch.float32, n)
say("dense kernels alone, n = 2^21 fp32 (HBM peak taken as 8 TB/s)")
say("%-22s %3s %3s %10s %10s %8s" % ("kernel", "m", "nk", "us", "GB/s", "of peak"))
Ks = [torch.randn(n, device=dev) for _ in range(6)]
u = torch.randn(n, device=dev)
for m in (1, 16, 32):
    out = torch.empty(m, n, device=dev)
    cf = [[0.01 * (j + 1) for j in range(6)] for _ in range(m)]
    Ds = [torch.empty(n, device=dev) for _ in range(6)]
    G = torch.empty(n, device=dev)
    for name, fn, nbytes in (("pn_rk_dense_eval", lambda: ops.dense_eval(out, u, Ks, cf), (6 + 1 + m) * n * 4),
                             ("pn_rk_dense_adjoint", lambda: ops.dense_adjoint(Ds, G, out, cf), (m + 6 + 1) * n * 4)):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 20
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / reps
        gbs = nbytes / us * 1e-3
        say("%-22s %3d %3d %10.1f %10.1f %7.2f" % (name, m, 6, us, gbs, gbs / 8000.0))
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
