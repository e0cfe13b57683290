"""Solve level: what -pn_linear_softplus 1 / -pn_linear_elu 1 is worth on a Linear -> Softplus / Linear -> ELU MLP of the headline's
shape (3 x [Linear(512, 512) + act] + Linear(512, 512) on 4096 x 512, rk4 x 100 steps of 0.01, forward + adjoint, graph mode as it is by
default), in ONE process (the method of tools/bench_linear_sigmoid.py):
     stock              no option
     bare               -pn_linear_bare 1                              (owned GEMMs, the activation's two launches of their own)
     bare+ACT           -pn_linear_bare 1 -pn_linear_ACT 1             (the pairs fused)
ROUNDS interleaved rounds: a round times CALLS training-style calls of every solver in turn (device-synchronised host clock), so that a
drift of the clocks falls on all alike.  Prints the median and the best round in time-steps/s and how far bare+ACT is from bare in the
relative 2-norm.
     python tools/bench_linear_softplus_elu.py softplus|elu [rounds [calls]]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

import pnode_amd  # noqa: F401
from pnode_amd import options, petsc_adjoint

NT, DT, BATCH, DIM = 100, 0.01, 4096, 512


ACTS = {"softplus": nn.Softplus, "elu": nn.ELU}


class MLP(nn.Module):
    def __init__(self, d, act, seed=0, std=0.02):
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
                layers.append(ACTS[act]())
        self.net = nn.Sequential(*layers)

    def forward(self, t, y):
        return self.net(y)


class Side(object):
    def __init__(self, name, opts, dev, act):
        self.name = name
        options.clear()
        for k, v in opts.items():
            options.set_option(k, v)
        self.f = MLP(DIM, act).to(dev)
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
    act = sys.argv[1] if len(sys.argv) > 1 else "softplus"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    dev = torch.device("cuda:0")
    both = "bare+" + act
    sides = [Side("stock", {"ts_adapt_type": "none"}, dev, act),
             Side("bare", {"ts_adapt_type": "none", "pn_linear_bare": 1}, dev, act),
             Side(both, {"ts_adapt_type": "none", "pn_linear_bare": 1, "pn_linear_" + act: 1}, dev, act)]
    for s in sides:                                # warm-up: the eager calls and the capturing one
        for _ in range(4):
            s.call()
    last = {}
    for _ in range(rounds):
        for s in sides:
            last[s.name] = s.block(calls)
    for s in sides:
        t = sorted(s.times)
        print("%-13s median %8.1f time-steps/s (best %8.1f, worst %8.1f) over %d rounds of %d calls; linear_%s: %s; linear_bare: %s; graphs: %s"
              % (s.name, t[len(t) // 2], t[-1], t[0], rounds, calls, act, getattr(s.ode, "linear_" + act), s.ode.linear_bare, s.ode.graph_status))
    print("%s against bare, relative 2-norm (solution, dL/dy0, dL/dtheta): %s"
          % (both, ["%.2e" % float((a - b).norm() / b.norm()) for a, b in zip(last[both], last["bare"])]))


if __name__ == "__main__":
    main()
