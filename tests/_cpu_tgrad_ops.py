"""TEST SCAFFOLDING -- the time-gradient entry points (pn_tgrad_dots / pn_rk_dense_tgrad, csrc/pn_tgrad.hip) on the CPU
stand-in of tests/_cpu_dense_ops.py: fp64 scalar products, accumulated into slots of an fp64 tensor."""
import torch

from _cpu_dense_ops import CpuDenseOps


class CpuTgradOps(CpuDenseOps):
    def tgrad_dots(self, acc, xs, ys, coefs, accumulate=True):
        self.calls["tgrad_dots"] = self.calls.get("tgrad_dots", 0) + 1
        n = self.n
        tot = torch.zeros((), dtype=torch.float64)
        for x, y, c in zip(xs, ys, coefs):
            tot = tot + c * torch.dot(x[:n].double(), y[:n].double())
        acc.copy_(acc + tot if accumulate else tot)

    def dense_tgrad(self, acc, g, Ks, coefs, accumulate=True):
        self.calls["dense_tgrad"] = self.calls.get("dense_tgrad", 0) + 1
        n = self.n
        for o, row in enumerate(coefs):
            tot = torch.zeros((), dtype=torch.float64)
            for k, c in zip(Ks, row):
                tot = tot + c * torch.dot(g[o][:n].double(), k[:n].double())
            acc[o] = acc[o] + tot if accumulate else tot
