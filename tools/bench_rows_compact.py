#!/usr/bin/env python3
"""-pn_rows_compact 1 against the option absent on a per-sample solve whose rows need spread step counts.

The batch is BASELINE's C3b-stiff shape cut to what fits a minute: --rows x 512 fp32 (default 2048), the C3 MLP, dopri5, forward +
adjoint over t = [0, 0.5, 1].  C3b-stiff itself needs 4 steps in every row (profiles/sample_adapt.txt), so here the rows carry a rate
in the last entry of their state -- f(y) = k * MLP(y with that entry masked) on the first 511 entries, dk/dt = 0 -- spread over
--decades decades (the MLP's own Lipschitz constant is about 0.04): the slow rows finish within a few rounds and the fast ones go
on for many.

Two arms, run ALTERNATELY --reps times after one warm-up solve each (as tools/mb_linear_bwd.py alternates its kernels), medians:
the option absent, and -pn_rows_compact 1 (passed in the second arm only).  Printed: the rows func was given against full-size
calls, forward and backward, and the two times.  On a tree without the option the second arm is the first again (unknown pn_* keys
are skipped) and the counters print as n/a: the first arm of that run is the baseline of this one's."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from pnode_amd import options, petsc_adjoint  # noqa: E402
from problems import MLPFunc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2048)
ap.add_argument("--decades", type=float, default=3.0)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tol", type=float, default=1e-4)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
D = 512


class RateMLP(nn.Module):
    def __init__(self):
        super().__init__()
        self.mlp = MLPFunc(D, torch.float32)
        self.register_buffer("mask", torch.cat([torch.ones(D - 1), torch.zeros(1)]))

    def forward(self, t, y):
        return self.mlp(t, y * self.mask) * (y[..., -1:] * self.mask)


def make(compact):
    g = torch.Generator().manual_seed(1)
    y0 = torch.randn(a.rows, D, generator=g) * 0.5
    y0[:, -1] = torch.logspace(0.0, a.decades, a.rows)
    options.clear()
    options.set_option("pn_adapt_scope", "sample")
    options.set_option("ts_rtol", a.tol)
    options.set_option("ts_atol", a.tol)
    if compact:
        options.set_option("pn_rows_compact", "1")
    ode = petsc_adjoint.ODEPetsc()
    y0 = y0.to(dev)
    ode.setupTS(y0, RateMLP().to(dev), step_size=0.01, method="dopri5")
    options.clear()
    return ode, y0


def run(ode, y0):
    t = torch.tensor([0.0, 0.5, 1.0], device=dev)
    y = y0.clone().requires_grad_(True)
    before = [getattr(ode, k, None) for k in ("rows_evaluated", "rows_evaluated_backward", "nfe_forward", "nfe_backward")]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol = ode.odeint_adjoint(y, t)
    sol.sum().backward()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    after = [getattr(ode, k, None) for k in ("rows_evaluated", "rows_evaluated_backward", "nfe_forward", "nfe_backward")]
    return ms, [None if x is None else y - x for x, y in zip(before, after)], sol.detach(), y.grad


arms = [("option absent", make(False)), ("-pn_rows_compact 1", make(True))]
for _, (ode, y0) in arms:
    run(ode, y0)
times, last = [[], []], [None, None]
for _ in range(a.reps):
    for k, (_, (ode, y0)) in enumerate(arms):
        ms, counts, sol, gu = run(ode, y0)
        times[k].append(ms)
        last[k] = (counts, sol, gu)

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ode = arms[0][1][0]
say("per-sample solve, %d x %d fp32, rates over %.1f decades, dopri5 tol %g, forward + adjoint; %d alternated runs, median [min .. max] ms"
    % (a.rows, D, a.decades, a.tol, a.reps))
say("rounds %d, accepted steps per row %d..%d, rejected %d..%d" % (ode.rounds, int(ode.sample_steps.min()), int(ode.sample_steps.max()),
                                                                 int(ode.sample_rejections.min()), int(ode.sample_rejections.max())))
for k, (name, (ode, _)) in enumerate(arms):
    rf, rb, nf, nb = last[k][0]
    full_f, full_b = a.rows * nf, a.rows * nb
    ratio = "rows evaluated n/a (no counters in this tree)" if rf is None else \
        "rows evaluated %d of %d forward (%.3f), %d of %d backward (%.3f)" % (rf, full_f, rf / full_f, rb, full_b, rb / max(full_b, 1))
    say("%-20s %9.2f [%8.2f .. %8.2f] ms   func calls %d + %d   %s" % (name, statistics.median(times[k]), min(times[k]), max(times[k]), nf, nb, ratio))
say("second arm / first arm: %.3f" % (statistics.median(times[1]) / statistics.median(times[0])))
say("second arm against first: max |sol| difference %.3e, max |dL/dy0| difference %.3e (relative to the largest entry)"
    % (float((last[1][1] - last[0][1]).abs().max() / last[0][1].abs().max()), float((last[1][2] - last[0][2]).abs().max() / last[0][2].abs().max())))
if a.out:
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
