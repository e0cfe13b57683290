#!/usr/bin/env python3
"""-pn_adapt_scope sample against batch at BASELINE's C3b shape (MLP 4096 x 512 fp32, dopri5 adaptive; C3b-stiff: initial rows
scaled over 1.5 decades) and the spiral 4096 x 2: rounds against steps, func evaluations, wall time per solve (forward +
adjoint; every solver is warmed --warmup calls first, which takes the batch path past the capture and validation of its
per-evaluation hipGraphs, then the median of --reps), and each pn_rows_* kernel next to its pn_* counterpart at 4096 x 512 fp32.

Kernel times come from a kernel trace, not from host-side brackets (a 6-12 us kernel is of the size of a launch gap):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/bench_sample_adapt.py --only-kernels
  python3 tools/bench_sample_adapt.py --from-trace DIR [--out FILE]          # (no device needed)

--only-kernels launches, per pair, the two kernels ALTERNATELY --launches times (and the counterpart a third time with the
plain launch policy, pn_tune_set "vpt=1,st=0", to tell a policy difference from a kernel difference); --from-trace takes each
kernel's durations from the trace in launch order, in 8 blocks: median, and spread = (max - min) / median of the block medians.
The one performance condition is relative: a pn_rows_* kernel moves one double per row more than its counterpart (8 B against
512 * 4 B per vector row, < 0.2 %), so its margin is 0.2 % plus the counterpart's spread.  The vectors of one launch (2-8 x 8 MiB)
stay inside the 256 MiB last-level cache between launches: the bytes/s column is algorithmic bytes over time, not HBM bandwidth.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--launches", type=int, default=400)
ap.add_argument("--out", default=None)
ap.add_argument("--only-kernels", action="store_true")
ap.add_argument("--only-solves", action="store_true")
ap.add_argument("--from-trace", default=None, metavar="DIR")
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish():
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


# (rows kernel, counterpart, algorithmic bytes of the pair at 4096 x 512 fp32) by the names the trace shows
N = 4096 * 512
PAIRS = [
    ("stage (6 K)", "pn_rows_lin_kernel<float, 6, true, true>", "pn_lincomb_kernel<float, 7,", 8 * N * 4),
    ("combine_wrms (6 K)", "pn_rows_combine_wrms_kernel<float, 6,", "pn_combine_wrms_kernel<float, 6,", 8 * N * 4),
    ("adj_theta (lam + 3)", "pn_rows_lin_kernel<float, 4, true, false>", "pn_lincomb_kernel<float, 4,", 5 * N * 4),
    ("adj_accum (5 dlam)", "pn_rows_adj_accum_kernel<float, 5,", "pn_lincomb_kernel<float, 6,", 7 * N * 4),
    ("commit / copy", "pn_rows_commit_kernel<float,", "pn_lincomb_kernel<float, 1,", 2 * N * 4),
]


def from_trace(d):
    import csv
    import glob
    import statistics
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Kernel_Name"]))
    rows.sort()
    if not rows:
        sys.exit("no kernel trace under " + d)

    def stat(pat, part=None):
        v = [us for _, us, n in rows if pat in n]
        if part is not None and v:                      # the counterpart runs twice per pair: tuned policy first, plain second
            half = len(v) // 2
            v = v[:half] if part == 0 else v[half:]
        v = v[len(v) // 10:]                            # (the first tenth: warm-up)
        if len(v) < 16:
            return None
        nb = 8
        meds = [statistics.median(v[i * len(v) // nb:(i + 1) * len(v) // nb]) for i in range(nb)]
        return statistics.median(v), (max(meds) - min(meds)) / statistics.median(meds), len(v)

    say("kernels at 4096 x 512 fp32 from a rocprofv3 kernel trace; alternated launches; median us; spread = (max - min) / median of 8 block medians")
    say("%-20s %9s %9s %11s %8s %8s %9s %9s  %s" % ("kernel", "rows us", "pn_* us", "pn_* plain", "spread", "margin", "rows TB/s", "pn_* TB/s", "verdict"))
    for name, rk, bk, nbytes in PAIRS:
        r, b0, b1 = stat(rk), stat(bk, 0), stat(bk, 1)
        if not (r and b0 and b1):
            say("%-20s not found in the trace (%s / %s)" % (name, rk, bk))
            continue
        margin = 0.002 + b0[1]
        ok = r[0] <= b0[0] * (1 + margin)
        say("%-20s %9.2f %9.2f %11.2f %7.1f%% %7.1f%% %9.2f %9.2f  %s" % (name, r[0], b0[0], b1[0], 100 * b0[1], 100 * margin, nbytes / r[0] * 1e-6,
                                                                       nbytes / b0[0] * 1e-6, "within" if ok else "OUTSIDE (%+.1f%%; against the plain policy %+.1f%%)"
                                                                       % (100 * (r[0] / b0[0] - 1), 100 * (r[0] / b1[0] - 1))))
    c = stat("pn_rows_control_kernel")
    if c:
        say("%-20s %9.2f   (one thread per row, B = 4096: no counterpart -- the batch path judges on the host; %d launches)" % ("control", c[0], c[2]))
    names = {}
    for _, us, n in rows:
        names.setdefault(n[:90], []).append(us)
    say("all kernels of the trace: " + "; ".join("%s x%d" % (k, len(v)) for k, v in sorted(names.items()) if "pn_" in k))


if a.from_trace:
    from_trace(a.from_trace)
    finish()
    sys.exit(0)

import torch  # noqa: E402
from pnode_amd import _lib, options, petsc_adjoint  # noqa: E402
from pnode_amd._vecops import HipVecOps  # noqa: E402
from problems import MLPFunc, SpiralFunc  # noqa: E402
dev = torch.device("cuda:0")


def problem(name):
    g = torch.Generator().manual_seed(1)
    if name == "spiral":
        f = SpiralFunc(torch.float32).to(dev)
        y0 = torch.randn(4096, 2, generator=g) * torch.logspace(-1, 0.3, 4096).view(-1, 1)
        return f, y0.to(dev), 1e-5
    f = MLPFunc(512, torch.float32).to(dev)
    y0 = torch.randn(4096, 512, generator=g) * 0.5
    if name == "C3b-stiff":
        y0 = y0 * torch.logspace(-1, 0.5, 4096).view(-1, 1)
    return f, y0.to(dev), 1e-4


def solve(name, scope, reps, tol_ref=None):
    f, y0, tol = problem(name)
    options.clear()
    options.set_option("pn_adapt_scope", scope)
    options.set_option("ts_rtol", tol_ref or tol)
    options.set_option("ts_atol", tol_ref or tol)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, f, step_size=0.01, method="dopri5")
    options.clear()
    t = torch.tensor([0.0, 0.5, 1.0], device=dev)
    times, sol = [], None
    for r in range(reps + (a.warmup if reps else 1)):
        y = y0.clone().requires_grad_(True)
        nf0, nb0 = ode.nfe_forward, ode.nfe_backward
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = ode.odeint_adjoint(y, t)
        sol.sum().backward()
        torch.cuda.synchronize()
        if reps and r >= a.warmup:
            times.append(time.perf_counter() - t0)
    ms = 1e3 * sorted(times)[len(times) // 2] if times else float("nan")
    n = ode.rounds if scope == "sample" else ode.num_steps
    return sol.detach(), n, ode.nfe_forward - nf0, ode.nfe_backward - nb0, ms, ode


if not a.only_kernels:
    say("forward + adjoint, t = [0, 0.5, 1], dopri5, %d warm-up calls then the median of %d; NFE of the last call; error = max per-row |y - y_ref| / max |y_ref|, "
        "y_ref: sample mode at tol/1000" % (a.warmup, a.reps))
    say("%-10s %-7s %14s %8s %8s %10s %12s  %s" % ("problem", "scope", "rounds/steps", "NFE-F", "NFE-B", "ms/solve", "max row err", "launches"))
    for name in ("C3b", "C3b-stiff", "spiral"):
        ref = solve(name, "sample", 0, tol_ref=problem(name)[2] * 1e-3)[0]
        for scope in ("batch", "sample"):
            sol, n, nf, nb, ms, ode = solve(name, scope, a.reps)
            err = float(((sol - ref).abs().amax(dim=(0, 2)) / ref.abs().max()).max())
            extra = "" if scope == "batch" else "; steps per row %d..%d" % (int(ode.sample_steps.min()), int(ode.sample_steps.max()))
            say("%-10s %-7s %14d %8d %8d %10.2f %12.3e  %s%s" % (name, scope, n, nf, nb, ms, err, ode.graph_status[:60], extra))

if not a.only_solves:
    B, d = 4096, 512
    n = B * d
    ops = HipVecOps(dev, torch.float32, n)
    K = [torch.randn(n, device=dev) for _ in range(6)]
    u, y, w = torch.randn(n, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    h = torch.full((B,), 0.01, dtype=torch.float64, device=dev)
    enorm = torch.empty(B, dtype=torch.float64, device=dev)
    acc = torch.ones(B, dtype=torch.int32, device=dev)
    hit = torch.full((B,), -1, dtype=torch.int32, device=dev)
    c6 = [0.1 * (j + 1) for j in range(6)]
    hc = [0.01 * c for c in c6]
    ops.wrms_buffers()
    launches = [
        (lambda: ops.rows_stage(B, d, y, u, K, c6, h), lambda: ops.rk_stage(y, u, K, hc)),
        (lambda: ops.rows_combine_wrms(B, d, y, u, K, c6, c6, h, 1e-4, 1e-4, enorm), lambda: ops.combine_wrms(y, u, K, hc, hc, 1e-4, 1e-4)),
        (lambda: ops.rows_adj_theta(B, d, w, u, 0.3, K[:3], c6[:3], h), lambda: ops.adj_theta(w, u, 0.003, K[:3], hc[:3])),
        (lambda: ops.rows_adj_accum(B, d, y, u, K[:5], None, 0, None, 0), lambda: ops.adj_accum(y, u, K[:5], [1.0] * 5, None)),
        (lambda: ops.rows_commit(B, d, y, u, w, acc, hit, None, 0, 0), lambda: ops.copy(y, w)),
    ]
    lib = ops.lib
    for rows_fn, base_fn in launches:
        for policy in (None, b"vpt=1,st=0,wvpt=1"):
            lib.pn_tune_set(policy)
            for _ in range(a.launches):
                if policy is None:
                    rows_fn()
                base_fn()
            torch.cuda.synchronize()
        lib.pn_tune_set(None)
    # the controller: B = 4096 rows, all unfinished and accepted
    import ctypes
    ts = ctypes.c_void_p(lib.pn_ts_create())
    lib.pn_ts_set_rk_type(ts, b"5dp")
    sd, si = ops.f64(_lib.PN_ROWS_ND, B), ops.i32(_lib.PN_ROWS_NI, B)
    sd[_lib.PN_ROWS_H].fill_(1e-6)
    en = torch.full((B,), 0.5, dtype=torch.float64, device=dev)
    log_d, log_hit, summary = ops.f64(3, B), ops.i32(B), ops.i32(4)
    for _ in range(a.launches):
        ops.rows_control(ts, B, 0, None, 1e9, en, sd, si, log_d, log_hit, acc, summary)
    torch.cuda.synchronize()
    lib.pn_ts_destroy(ts)
    say("kernel launches done (%d per kernel, alternated): take the times from the kernel trace with --from-trace" % a.launches)
finish()
