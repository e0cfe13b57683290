#!/usr/bin/env python3
"""The infinity-norm kernels (-ts_adapt_wnormtype infinity) next to the kernels they stand beside, on the same operands:
pn_rk_combine_winf against pn_rk_combine_wrms and pn_rows_combine_winf against pn_rows_combine_wrms at 4096 x 512, fp32 and
fp64, seven stage derivatives, the writing form (unew stored).  The comparators are unchanged code and both kernels of a pair
move the same bytes, so parity is what to expect.

Times come from HIP events around runs of --burst back-to-back launches of ONE kernel, the two kernels of a pair taking turns
(A burst, B burst, A burst, ...), so that clock and cache state drift hits both alike; a burst's time over its launches is one
sample.  Per kernel: the median of the samples after the first tenth (warm-up), and spread = (max - min) / median of the medians
of 8 consecutive blocks of samples.  The margin of a pair is the comparator's own spread plus 0.2 % (the rule of
profiles/sample_adapt.txt).  The vectors of one launch (9 x 8 or 16 MiB) stay inside the 256 MiB last-level cache between
launches: the TB/s column is algorithmic bytes over time, not HBM bandwidth.

  python3 tools/bench_winf_norm.py [--out profiles/winf_norm.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--bursts", type=int, default=160, help="samples per kernel")
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
    """us per launch of each of `fns`, taking turns burst by burst."""
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


say("error-norm kernels at %d x %d, nk = %d, writing form; HIP events around bursts of %d launches, kernels of a pair taking turns, "
    "%d samples each; median us per launch; spread = (max - min) / median of 8 block medians; margin = comparator's spread + 0.2 %%"
    % (B, d, NK, a.burst, a.bursts))
say("%-34s %10s %10s %8s %8s %9s %9s  %s" % ("pair", "winf us", "wrms us", "spread", "margin", "winf TB/s", "wrms TB/s", "verdict"))
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
    nbytes = (NK + 2) * n * u.element_size()
    pairs = [
        ("pn_rk_combine_w{inf,rms}", lambda: ops.combine_winf(y, u, K, hc, hc, 1e-4, 1e-4), lambda: ops.combine_wrms(y, u, K, hc, hc, 1e-4, 1e-4)),
        ("pn_rows_combine_w{inf,rms}", lambda: ops.rows_combine_winf(B, d, y, u, K, c, c, h, 1e-4, 1e-4, enorm),
         lambda: ops.rows_combine_wrms(B, d, y, u, K, c, c, h, 1e-4, 1e-4, enorm)),
    ]
    for name, new_fn, old_fn in pairs:
        tn, to = timed([new_fn, old_fn])
        (mn, sn), (mo, so) = stat(tn), stat(to)
        margin = 0.002 + so
        ok = mn <= mo * (1 + margin)
        say("%-34s %10.2f %10.2f %7.1f%% %7.1f%% %9.2f %9.2f  %s"
            % (name + " " + str(dtype).replace("torch.", ""), mn, mo, 100 * so, 100 * margin, nbytes / mn * 1e-6, nbytes / mo * 1e-6,
               "within" if ok else "OUTSIDE (%+.1f%%)" % (100 * (mn / mo - 1))))
    del ops, K, u, y
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
