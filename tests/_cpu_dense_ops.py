"""TEST SCAFFOLDING -- the dense-output entry points (pn_rk_dense_eval / pn_rk_dense_adjoint, csrc/pn_dense.hip) on the CPU
stand-in of tests/_cpu_vecops.py, in the kernels' order: out_o = u, then + c_oj K_j in j order; D_j = c_0j g_0, then + c_oj g_o
in o order; G = g_0 + g_1 + ...  (accumulate: from what is there)."""
import torch

from _cpu_vecops import CpuVecOps


class CpuDenseOps(CpuVecOps):
    def dense_eval(self, out, u, Ks, coefs):
        self.calls["dense_eval"] = self.calls.get("dense_eval", 0) + 1
        n = self.n
        for o, row in enumerate(coefs):
            acc = u[:n].clone()
            for k, c in zip(Ks, row):
                acc = acc + c * k[:n]
            self._put(out[o], acc)

    def dense_adjoint(self, Ds, G, g, coefs, accumulate=False):
        self.calls["dense_adjoint"] = self.calls.get("dense_adjoint", 0) + 1
        n = self.n
        d = [x[:n].clone() for x in Ds] if accumulate else None
        s = G[:n].clone() if (accumulate and G is not None) else None
        for o, row in enumerate(coefs):
            go = g[o][:n]
            if d is None:
                d = [c * go for c in row]
            else:
                d = [dj + c * go for dj, c in zip(d, row)]
            s = go.clone() if s is None else s + go
        for x, v in zip(Ds, d):
            self._put(x, v)
        if G is not None:
            self._put(G, s)
