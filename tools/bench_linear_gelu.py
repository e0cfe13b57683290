"""Solve level: what -pn_linear_gelu 1 is worth on a Linear -> GELU MLP of the headline's shape (3 x [Linear(512, 512) + GELU]
+ Linear(512, 512) on 4096 x 512, rk4 x 100 steps of 0.01, forward + adjoint, graph mode as it is by default), in ONE process:
     stock              no option
     bare               -pn_linear_bare 1                         (owned GEMMs, gelu and gelu_backward launches of their own)
     bare+gelu       -pn_linear_bare 1 -pn_linear_gelu 1    (the pairs fused)
ROUNDS interleaved rounds: a round times CALLS training-style calls of every solver in turn (device-synchronised host clock), so that a
drift of the clocks falls on all alike.  Prints the median and the best round in time-steps/s and how far bare+gelu is from bare in
the relative 2-norm (the kernel's GELU is not F.gelu's bit for bit).
     python tools/bench_linear_gelu.py [rounds [calls]]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import pnode_amd  # noqa: F401
from pnode_amd import options, petsc_adjoint

NT, DT, BATCH, DIM = 100, 0.01, 4096, 512


class GeluMLP(nn.Module):
    def __init__(self, d, seed=0, std=0.02):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        layers = []
        for k in range(4):
            lin = nn.Linear(d, d)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(d, d, generator=g) * std)
                lin.bias.zero_()
            layers.append(lin)
            if k < 3:
                layers.append(nn.GELU())
        self.net = nn.Sequential(*layers)

    def forward(self, t, y):
        return self.net(y)


class Side(object):
    def __init__(self, name, opts, dev):
        self.name = name
        options.clear()
        for k, v in opts.items():
            options.set_option(k, v)
        self.f = GeluMLP(DIM).to(dev)
        self.y0 = torch.randn(BATCH, DIM, generator=torch.Generator().manual_seed(1)).to(dev)
        self.t = torch.tensor([0.0, NT * DT], dtype=torch.float64, device=dev)
        self.ode = petsc_adjoint.ODEPetsc()
        self.ode.setupTS(self.y0, self.f, step_size=DT, method="rk4")
        options.clear()
        self.times = []

    def call(self):
        for p in self.f.parameters():
            p.grad = None
        y = self.y0.clone().requires_grad_(True)
        sol = self.ode.odeint_adjoint(y, self.t)
        sol[-1].pow(2).sum().backward()
        return sol.detach(), y.grad, torch.cat([p.grad.reshape(-1) for p in self.f.parameters()])

    def block(self, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = self.call()
        torch.cuda.synchronize()
        self.times.append(calls * NT / (time.perf_counter() - t0))
        return out


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda:0")
    sides = [Side("stock", {"ts_adapt_type": "none"}, dev),
             Side("bare", {"ts_adapt_type": "none", "pn_linear_bare": 1}, dev),
             Side("bare+gelu", {"ts_adapt_type": "none", "pn_linear_bare": 1, "pn_linear_gelu": 1}, dev)]
    for s in sides:                                # warm-up: the eager calls and the capturing one
        for _ in range(4):
            s.call()
    last = {}
    for _ in range(rounds):
        for s in sides:
            last[s.name] = s.block(calls)
    for s in sides:
        t = sorted(s.times)
        print("%-10s median %8.1f time-steps/s (best %8.1f, worst %8.1f) over %d rounds of %d calls; linear_gelu: %s; linear_bare: %s; graphs: %s"
              % (s.name, t[len(t) // 2], t[-1], t[0], rounds, calls, s.ode.linear_gelu, s.ode.linear_bare, s.ode.graph_status))
    print("bare+gelu against bare, relative 2-norm (solution, dL/dy0, dL/dtheta): %s"
          % ["%.2e" % float((a - b).norm() / b.norm()) for a, b in zip(last["bare+gelu"], last["bare"])])


if __name__ == "__main__":
    main()
