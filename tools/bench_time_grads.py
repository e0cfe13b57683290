"""Cost of dL/dt: forward + backward of odeint_adjoint with and without t.requires_grad, eager
(-pn_graph_capture 0), at the C3a shape (4096 x 512 fp32 MLP, rk4, h = 0.01, t = [0, 1]) and on the spiral demo under dopri5
with 1001 interpolated outputs; plus the default launch mode, where a solve whose t requires grad declines capture.
Writes profiles/time_grads.txt.  Usage: python tools/bench_time_grads.py [--reps R] [--quick]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnode_amd  # noqa: E402,F401  (before the first HIP call)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from pnode_amd import options, petsc_adjoint  # noqa: E402
from problems import SpiralFunc  # noqa: E402

DEV = torch.device("cuda:0")


class C3aFunc(nn.Module):
    def __init__(self, d=512):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(d, d), nn.Tanh(), nn.Linear(d, d))

    def forward(self, t, y):
        return self.net(y)


def run(func, y0, t, method, step, opts, t_grad, reps, warm=3):
    options.clear()
    for k, v in opts:
        options.set_option(k, v)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, func, step_size=step, method=method)
    times = []
    for r in range(warm + reps):
        yy = y0.clone().requires_grad_(True)
        tt = t.clone().requires_grad_(t_grad)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = ode.odeint_adjoint(yy, tt)
        y.sum().backward()
        torch.cuda.synchronize()
        if r >= warm:
            times.append(time.perf_counter() - t0)
    status = ode.graph_status
    options.clear()
    return statistics.median(times) * 1e3, status


class C3aTimeFunc(C3aFunc):
    """The same MLP with a time-dependent gain read through torch ops: every stage then has a t-path (T-bar != 0)."""

    def forward(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        return self.net(y) * (1.0 + 0.1 * torch.sin(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="two reps per case, nothing written (for a kernel trace)")
    a = ap.parse_args()
    torch.manual_seed(0)
    lines = ["# dL/dt cost: median ms of forward + backward over %d reps (after 3 warm-up calls), %s" % (a.reps, torch.cuda.get_device_name(0)),
             "# eager rows: two interleaved rounds (without, with, without, with); 'noise' is the difference between the two rounds'",
             "# medians of the same configuration, relative -- an overhead smaller than it is not resolved"]
    y0c, tc = torch.randn(4096, 512, device=DEV), torch.tensor([0.0, 1.0], device=DEV)
    c3a = (C3aFunc().to(DEV), y0c, tc, "rk4", 0.01, (("ts_adapt_type", "none"),))
    c3at = (C3aTimeFunc().to(DEV), y0c, tc, "rk4", 0.01, (("ts_adapt_type", "none"),))
    spiral = (SpiralFunc(dtype=torch.float32).to(DEV), torch.randn(1000, 1, 2, device=DEV) * 0.5,
              torch.linspace(0.0, 5.0, 1001, device=DEV), "dopri5", 0.025, (("pn_output_times", "interpolate"),))
    cases = [("C3a 4096x512 fp32 rk4 h=0.01 (autonomous)", c3a), ("C3a, func reads t (torch ops)", c3at),
             ("spiral dopri5, 1001 interpolated outputs", spiral)]
    reps = 2 if a.quick else a.reps
    for name, (f, y0, t, m, h, opts) in cases:
        eager = opts + (("pn_graph_capture", "0"),)
        rounds = 1 if a.quick else 2
        offs, ons = [], []
        for _ in range(rounds):
            offs.append(run(f, y0, t, m, h, eager, False, reps)[0])
            ons.append(run(f, y0, t, m, h, eager, True, reps)[0])
        off, on = statistics.mean(offs), statistics.mean(ons)
        noise = max(abs(offs[-1] - offs[0]) / off, abs(ons[-1] - ons[0]) / on)
        lines.append("%-44s eager: without t grad %8.2f ms   with %8.2f ms   overhead %+6.1f %%   noise %.1f %%"
                     % (name, off, on, 100 * (on / off - 1), 100 * noise))
        if not a.quick:
            doff, soff = run(f, y0, t, m, h, opts, False, reps)
            don, son = run(f, y0, t, m, h, opts, True, reps)
            lines.append("%-44s default: without %8.2f ms [%s]   with %8.2f ms [%s]   %+6.1f %%"
                         % ("", doff, soff, don, son, 100 * (don / doff - 1)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if not a.quick:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "time_grads.txt"), "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
