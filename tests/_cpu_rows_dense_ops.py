"""TEST SCAFFOLDING -- the row-dense entry points (pn_rows_dense_eval, pn_rows_dense_adjoint, pn_rows_adj_theta_dense;
csrc/pn_rows.hip) on the CPU stand-in of tests/_cpu_rows_ops.py.  Which outputs a row serves in a round and the coefficients
h_r beta_j(theta) are the product's own text run on host arrays (pn_rows_dense_plan_host); the arithmetic on the rows is in
the kernels' order: u first, then c_j K_j in j order; D_j from zero, + c_oj g_o with o ascending; G = g_lo + ...; the stage
cotangent's D_i added last."""
import torch

from pnode_amd import _lib

from _cpu_rows_ops import CpuRowsOps


class CpuRowsDenseOps(CpuRowsOps):
    rows_dense = True

    def _plan(self, B, nout, times, log_d, tnew, log_hit, nxt, rng, nk, P):
        coef = torch.zeros(nout, B, nk, dtype=torch.float64)
        lib = _lib.load()
        _lib.check(lib.pn_rows_dense_plan_host(B, nout, times.data_ptr(), log_d.data_ptr(), None if tnew is None else tnew.data_ptr(),
                                               None if log_hit is None else log_hit.data_ptr(), None if nxt is None else nxt.data_ptr(),
                                               rng.data_ptr(), nk, P, coef.data_ptr()))
        return coef

    def rows_dense_eval(self, B, d, sol, times, u, Ks, P, unew, log_d, tnew, log_hit, nxt, rng):
        self.calls["rows_dense_eval"] = self.calls.get("rows_dense_eval", 0) + 1
        nout = sol.shape[0]
        assert tnew.is_contiguous() and log_d.is_contiguous() and rng.is_contiguous()
        coef = self._plan(B, nout, times, log_d, tnew, log_hit, nxt, rng, len(Ks), P)
        ur, un = self._rows(u, B, d), self._rows(unew, B, d)
        kr = [self._rows(k, B, d) for k in Ks]
        out = sol.detach().numpy()
        for r in range(B):
            for o in range(int(rng[0, r]), int(rng[1, r])):
                acc = ur[r].clone()
                for j, k in enumerate(kr):
                    acc = acc + coef[o, r, j].to(self.dtype) * k[r]
                out[o].reshape(-1)[r * d:(r + 1) * d] = acc.numpy()
            if int(log_hit[r]) >= 0:
                out[int(log_hit[r])].reshape(-1)[r * d:(r + 1) * d] = un[r].numpy()

    def rows_dense_adjoint(self, B, d, Ds, G, g, times, P, rng, log_d):
        self.calls["rows_dense_adjoint"] = self.calls.get("rows_dense_adjoint", 0) + 1
        nout = g.shape[0]
        coef = self._plan(B, nout, times, log_d, None, None, None, rng, len(Ds), P)
        D = torch.zeros(len(Ds), B, d, dtype=self.dtype)
        S = torch.zeros(B, d, dtype=self.dtype)
        for r in range(B):
            for o in range(int(rng[0, r]), int(rng[1, r])):
                go = g.detach()[o].reshape(-1)[r * d:(r + 1) * d]
                for j in range(len(Ds)):
                    D[j, r] = D[j, r] + coef[o, r, j].to(self.dtype) * go
                S[r] = S[r] + go
        for x, v in zip(Ds, D):
            self._rput(x, v, B, d)
        self._rput(G, S, B, d)

    def rows_adj_theta(self, B, d, w, lam, c_lam, dlams, coefs, h, dense_w=None):
        if dense_w is None:
            return super().rows_adj_theta(B, d, w, lam, c_lam, dlams, coefs, h)
        self.calls["rows_adj_theta_dense"] = self.calls.get("rows_adj_theta_dense", 0) + 1
        xs = ([lam] if lam is not None else []) + list(dlams)
        cs = ([c_lam] if lam is not None else []) + list(coefs)
        self._rput(w, self._rlin(B, d, None, xs, cs, h) + self._rows(dense_w, B, d), B, d)
