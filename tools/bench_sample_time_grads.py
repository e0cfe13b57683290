#!/usr/bin/env python3
"""Cost of dL/dt under -pn_adapt_scope sample at BASELINE's C3b shape (MLP 4096 x 512 fp32, dopri5
adaptive, t = [0, 0.5, 1]): forward + backward with and without t.requires_grad (median of --reps after --warmup calls, two
interleaved rounds; 'noise' is the difference between the rounds' medians of one configuration), and pn_rows_tgrad_dots next to
pn_tgrad_dots on the same bytes (one pair of 4096 x 512 fp32 vectors).

Kernel times come from a kernel trace, not from host-side brackets:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/bench_sample_time_grads.py --only-kernels
  python3 tools/bench_sample_time_grads.py --from-trace DIR --append          # (no device needed)

--only-kernels launches the two kernels ALTERNATELY --launches times; --from-trace takes each kernel's durations in launch order,
in 8 blocks: median, and spread = (max - min) / median of the block medians.  The margin is the one profiles/sample_adapt.txt set
for row kernels against their counterparts: 0.2 % plus the counterpart's measured spread.  Writes profiles/sample_time_grads.txt."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
OUT = os.path.join(ROOT, "profiles", "sample_time_grads.txt")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--launches", type=int, default=400)
ap.add_argument("--only-kernels", action="store_true")
ap.add_argument("--from-trace", default=None, metavar="DIR")
ap.add_argument("--append", action="store_true", help="add to profiles/sample_time_grads.txt instead of replacing it")
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a" if a.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")


N = 4096 * 512
ROWS, BASE = "pn_rows_tgrad_dots_kernel<float, 1,", "pn_tgrad_dots_kernel<float, 1,"

if a.from_trace:
    import csv
    import glob
    rows = []
    for f in glob.glob(a.from_trace + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Kernel_Name"]))
    rows.sort()

    def stat(pat):
        v = [us for _, us, n in rows if pat in n]
        v = v[len(v) // 10:]                            # (the first tenth: warm-up)
        if len(v) < 16:
            return None
        meds = [statistics.median(v[i * len(v) // 8:(i + 1) * len(v) // 8]) for i in range(8)]
        return statistics.median(v), (max(meds) - min(meds)) / statistics.median(meds), len(v)

    r, b = stat(ROWS), stat(BASE)
    if not (r and b):
        sys.exit("pn_rows_tgrad_dots / pn_tgrad_dots not found in the kernel trace under " + a.from_trace)
    margin = 0.002 + b[1]
    say("kernels on one pair of 4096 x 512 fp32 vectors (16 MiB) from a rocprofv3 kernel trace; alternated launches; median us")
    say("pn_rows_tgrad_dots %.2f us (%.2f TB/s)   pn_tgrad_dots %.2f us (%.2f TB/s)   spread %.1f %%   margin %.1f %%   %s"
        % (r[0], 2 * N * 4 / r[0] * 1e-6, b[0], 2 * N * 4 / b[0] * 1e-6, 100 * b[1], 100 * margin,
           "within" if r[0] <= b[0] * (1 + margin) else "OUTSIDE (%+.1f %%)" % (100 * (r[0] / b[0] - 1))))
    finish()
    sys.exit(0)

import torch  # noqa: E402
from pnode_amd import options, petsc_adjoint  # noqa: E402
from pnode_amd._vecops import HipVecOps  # noqa: E402
from problems import MLPFunc  # noqa: E402
dev = torch.device("cuda:0")

if a.only_kernels:
    B, d = 4096, 512
    ops = HipVecOps(dev, torch.float32, N)
    x, y = torch.randn(N, device=dev), torch.randn(N, device=dev)
    rowacc, acc = ops.f64(B), ops.f64(1)
    for _ in range(a.launches):
        ops.rows_tgrad_dots(B, d, rowacc, [x], [y], [1.0], accumulate=True)
        ops.tgrad_dots(acc, [x], [y], [1.0])
    torch.cuda.synchronize()
    print("kernel launches done (%d per kernel, alternated): take the times from the kernel trace with --from-trace" % a.launches)
    sys.exit(0)


def run(t_grad, reps):
    g = torch.Generator().manual_seed(1)
    f = MLPFunc(512, torch.float32).to(dev)
    y0 = (torch.randn(4096, 512, generator=g) * 0.5).to(dev)
    options.clear()
    options.set_option("pn_adapt_scope", "sample")
    options.set_option("ts_rtol", 1e-4)
    options.set_option("ts_atol", 1e-4)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, f, step_size=0.01, method="dopri5")
    options.clear()
    fwd, bwd = [], []
    for r in range(a.warmup + reps):
        y = y0.clone().requires_grad_(True)
        t = torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64, device=dev, requires_grad=t_grad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = ode.odeint_adjoint(y, t)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sol.sum().backward()
        torch.cuda.synchronize()
        if r >= a.warmup:
            fwd.append(t1 - t0)
            bwd.append(time.perf_counter() - t1)
    return 1e3 * statistics.median(fwd), 1e3 * statistics.median(bwd), ode.rounds


say("# dL/dt under -pn_adapt_scope sample, C3b shape (4096 x 512 fp32 MLP, dopri5, tol 1e-4, t = [0, 0.5, 1]), %s" % torch.cuda.get_device_name(0))
say("# median ms over %d reps after %d warm-up calls; two interleaved rounds; noise = difference between the rounds, relative" % (a.reps, a.warmup))
offs, ons = [], []
for _ in range(2):
    offs.append(run(False, a.reps))
    ons.append(run(True, a.reps))
off, on = statistics.mean(o[1] for o in offs), statistics.mean(o[1] for o in ons)
noise = max(abs(offs[1][1] - offs[0][1]) / off, abs(ons[1][1] - ons[0][1]) / on)
say("backward: without t grad %8.2f ms   with %8.2f ms   overhead %+6.1f %%   noise %.1f %%   (%d rounds; forward %.2f / %.2f ms)"
    % (off, on, 100 * (on / off - 1), 100 * noise, ons[0][2], statistics.mean(o[0] for o in offs), statistics.mean(o[0] for o in ons)))
finish()
