#!/usr/bin/env python3
"""The per-component error-norm kernels (ODEPetsc.setTolerances) next to their scalar counterparts, on the
same operands and in the same process: pn_rk_combine_wrms_v / pn_rk_combine_winf_v against pn_rk_combine_wrms / pn_rk_combine_winf
at 4096 x 512 with period 512 (one sample) and period n (the whole state), and pn_rows_combine_wrms_v / pn_rows_combine_winf_v
against their counterparts (period d = 512), fp32 and fp64, seven stage derivatives, the writing form.

Expectation: period 512 reads 8 KiB of tolerances per workgroup from L1 / L2 and adds no HBM traffic -- parity within the
spread; period n reads two more fp64 vectors of n entries beside the nine state-sized ones: +2*8 / (9*4) = +44 % bytes at
fp32, +22 % at fp64.

Method as tools/bench_winf_norm.py: HIP events around bursts of --burst back-to-back launches of ONE kernel, the kernels of a
group taking turns burst by burst; per kernel the median of the samples after the first tenth, spread = (max - min) / median
of the medians of 8 consecutive blocks of samples.  The vectors of one launch stay inside the 256 MiB last-level cache between
launches: ratios compare like with like, the TB/s figure is algorithmic bytes over time, not HBM bandwidth.

  python3 tools/bench_vector_tolerances.py [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--bursts", type=int, default=120, help="samples per kernel")
ap.add_argument("--burst", type=int, default=10, help="launches per sample")
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import torch  # noqa: E402
from pnode_amd._vecops import HipVecOps  # noqa: E402

dev = torch.device("cuda:0")
B, d, NK = 4096, 512, 7
n = B * d


def stat(v):
    v = v[len(v) // 10:]
    nb = 8
    meds = [statistics.median(v[i * len(v) // nb:(i + 1) * len(v) // nb]) for i in range(nb)]
    return statistics.median(v), (max(meds) - min(meds)) / statistics.median(meds)


def timed(fns):
    out = [[] for _ in fns]
    for _ in range(a.bursts):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.burst):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(1e3 * e0.elapsed_time(e1) / a.burst)
    return out


say("error-norm kernels at %d x %d, nk = %d, writing form; HIP events around bursts of %d launches, the kernels of a group taking "
    "turns, %d samples each; median us per launch; spread = (max - min) / median of 8 block medians of the scalar kernel"
    % (B, d, NK, a.burst, a.bursts))
say("%-40s %10s %10s %8s %8s" % ("kernel (against its scalar counterpart)", "us", "scalar us", "ratio", "spread"))
for dtype in (torch.float32, torch.float64):
    ops = HipVecOps(dev, dtype, n)
    g = torch.Generator(device=dev).manual_seed(1)
    K = [torch.randn(n, dtype=dtype, device=dev, generator=g) for _ in range(NK)]
    u = torch.randn(n, dtype=dtype, device=dev, generator=g)
    y = torch.empty(n, dtype=dtype, device=dev)
    h = torch.full((B,), 0.01, dtype=torch.float64, device=dev)
    enorm = torch.empty(B, dtype=torch.float64, device=dev)
    c = [0.1 * (j + 1) for j in range(NK)]
    hc = [0.01 * x for x in c]
    ops.wrms_buffers()
    va = {p: torch.full((p,), 1e-4, dtype=torch.float64, device=dev) for p in (d, n)}
    vr = {p: torch.full((p,), 1e-4, dtype=torch.float64, device=dev) for p in (d, n)}
    tname = str(dtype).replace("torch.", "")
    groups = [
        ("pn_rk_combine_wrms", lambda: ops.combine_wrms(y, u, K, hc, hc, 1e-4, 1e-4),
         [("_v p = 512", lambda: ops.combine_wrms_v(y, u, K, hc, hc, va[d], vr[d])),
          ("_v p = n", lambda: ops.combine_wrms_v(y, u, K, hc, hc, va[n], vr[n]))]),
        ("pn_rk_combine_winf", lambda: ops.combine_winf(y, u, K, hc, hc, 1e-4, 1e-4),
         [("_v p = 512", lambda: ops.combine_winf_v(y, u, K, hc, hc, va[d], vr[d])),
          ("_v p = n", lambda: ops.combine_winf_v(y, u, K, hc, hc, va[n], vr[n]))]),
        ("pn_rows_combine_wrms", lambda: ops.rows_combine_wrms(B, d, y, u, K, c, c, h, 1e-4, 1e-4, enorm),
         [("_v p = d = 512", lambda: ops.rows_combine_wrms_v(B, d, y, u, K, c, c, h, va[d], vr[d], enorm))]),
        ("pn_rows_combine_winf", lambda: ops.rows_combine_winf(B, d, y, u, K, c, c, h, 1e-4, 1e-4, enorm),
         [("_v p = d = 512", lambda: ops.rows_combine_winf_v(B, d, y, u, K, c, c, h, va[d], vr[d], enorm))]),
    ]
    for name, old_fn, news in groups:
        ts = timed([old_fn] + [fn for _, fn in news])
        mo, so = stat(ts[0])
        for (label, _), t in zip(news, ts[1:]):
            mn, _ = stat(t)
            say("%-40s %10.2f %10.2f %8.3f %7.1f%%" % ("%s%s %s" % (name, label, tname), mn, mo, mn / mo, 100 * so))
    del ops, K, u, y
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
