"""TEST SCAFFOLDING -- the per-sample entry points (pn_rows_*, csrc/pn_rows.hip) on the CPU stand-in of
tests/_cpu_tgrad_ops.py.  The arithmetic order mirrors the kernels (coefficients h_r * c_j formed in double and rounded once,
u first, then one term after the other); the per-row controller is the product's own text run on host arrays
(pn_rows_control_host)."""
import torch

from oracle import ts_oracle
from pnode_amd import _lib

from _cpu_tgrad_ops import CpuTgradOps


class CpuRowsOps(CpuTgradOps):
    def f64(self, *shape):
        return torch.zeros(*shape, dtype=torch.float64)

    def i32(self, *shape):
        return torch.zeros(*shape, dtype=torch.int32)

    def _rows(self, x, B, d):
        return x.detach()[: B * d].view(B, d)

    def _rput(self, dst, val, B, d):
        dst.detach().numpy()[: B * d] = val.reshape(-1).numpy()

    def _rlin(self, B, d, base, xs, cs, h):
        hc = h.detach().view(B, 1)
        acc = None if base is None else self._rows(base, B, d).clone()
        for x, c in zip(xs, cs):
            term = (hc * c).to(self.dtype) * self._rows(x, B, d)
            acc = term if acc is None else acc + term
        return acc

    def rows_stage(self, B, d, y, u, Ks, coefs, h):
        self.calls["rows_stage"] = self.calls.get("rows_stage", 0) + 1
        self._rput(y, self._rlin(B, d, u, Ks, coefs, h), B, d)

    def rows_combine_wrms(self, B, d, unew, u, Ks, cb, ce, h, atol, rtol, enorm):
        self.calls["rows_combine_wrms"] = self.calls.get("rows_combine_wrms", 0) + 1
        if unew is not None:
            un = self._rlin(B, d, u, Ks, cb, h)
            self._rput(unew, un, B, d)
        else:
            un = self._rows(u, B, d).clone()
        err = self._rlin(B, d, None, Ks, ce, h)
        uh = (un + err).to(self.dtype)
        for r in range(B):
            enorm[r] = ts_oracle.wrms(un[r].numpy(), uh[r].numpy(), atol, rtol)

    def rows_control(self, ts, B, nspan, span, max_time, enorm, sd, si, log_d, log_hit, accept, summary):
        self.calls["rows_control"] = self.calls.get("rows_control", 0) + 1
        lib = _lib.load()
        _lib.check(lib.pn_rows_control_host(ts, B, nspan, None if span is None else span.data_ptr(), max_time, enorm.data_ptr(),
                                            sd.data_ptr(), si.data_ptr(), log_d.data_ptr(), log_hit.data_ptr(), accept.data_ptr(),
                                            summary.data_ptr()))

    def rows_summary(self, summary):
        self.calls["rows_summary"] = self.calls.get("rows_summary", 0) + 1
        v = summary.tolist()
        return v[0], v[1], v[2]

    def rows_commit(self, B, d, unext, u, unew, accept, hit, sol, ld, nout):
        self.calls["rows_commit"] = self.calls.get("rows_commit", 0) + 1
        acc = accept.bool().view(B, 1)
        un = self._rows(unew, B, d)
        self._rput(unext, torch.where(acc, un, self._rows(u, B, d)), B, d)
        if sol is not None:
            for r in range(B):
                if accept[r] and 0 <= int(hit[r]) < nout:
                    sol.detach().numpy()[int(hit[r])].reshape(B, d)[r] = un[r].numpy()

    def rows_adj_theta(self, B, d, w, lam, c_lam, dlams, coefs, h):
        self.calls["rows_adj_theta"] = self.calls.get("rows_adj_theta", 0) + 1
        xs = ([lam] if lam is not None else []) + list(dlams)
        cs = ([c_lam] if lam is not None else []) + list(coefs)
        self._rput(w, self._rlin(B, d, None, xs, cs, h), B, d)

    def rows_adj_accum(self, B, d, lam_out, lam, dlams, g, ld, hit, nout):
        self.calls["rows_adj_accum"] = self.calls.get("rows_adj_accum", 0) + 1
        acc = self._rows(lam, B, d).clone()
        for x in dlams:
            acc = acc + self._rows(x, B, d)
        if g is not None:
            for r in range(B):
                if 0 <= int(hit[r]) < nout:
                    acc[r] = acc[r] + g.detach()[int(hit[r])].view(B, d)[r]
        self._rput(lam_out, acc, B, d)
