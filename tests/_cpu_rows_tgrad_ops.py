"""TEST SCAFFOLDING -- the per-sample time-gradient entry points (pn_rows_tgrad_dots, pn_rows_dense_tgrad, pn_rows_tgrad_scatter,
pn_rows_tgrad_reduce; csrc/pn_rows.hip) on the CPU stand-in of tests/_cpu_rows_dense_ops.py.  theta, beta' and the per-row scatter
are the product's own text run on host arrays (pn_rows_dense_tgrad_host, pn_rows_tgrad_scatter_host); the sums are taken in the
kernels' order: a row's chunks of 16 bytes dealt to the G threads of its group, per thread in ascending order, then the halving
tree inside a wave and the waves in order; over the rows, 256 columns per workgroup, the block tree, the partials in index order."""
import ctypes

import torch

from pnode_amd import _lib

from _cpu_rows_dense_ops import CpuRowsDenseOps

_BLOCK, _WAVE, _REDUCE_BLOCKS = 256, 64, 64


def _tree(v):
    """lane 0 of `for o = n/2 .. 1: v[i] += v[i + o]` (n a power of two)"""
    v = list(v)
    while len(v) > 1:
        half = len(v) // 2
        v = [v[i] + v[i + half] for i in range(half)]
    return v[0]


def _group_sum(per_thread):
    G = len(per_thread)
    if G <= _WAVE:
        return _tree(per_thread)
    tot = 0.0
    for w in range(G // _WAVE):
        tot = tot + _tree(per_thread[w * _WAVE:(w + 1) * _WAVE])
    return tot


def _block_sum(per_thread):
    return _group_sum(list(per_thread) + [0.0] * (_BLOCK - len(per_thread)))


class CpuRowsTgradOps(CpuRowsDenseOps):
    rows_tgrad = True

    def _geom(self, d):
        vw = 16 // torch.empty((), dtype=self.dtype).element_size()
        nch = (d + vw - 1) // vw
        G = 1
        while G < nch and G < _BLOCK:
            G *= 2
        return vw, nch, G

    def _row_sum(self, d, chunk_term):
        """sum over the row's chunks of chunk_term(first element, one past the last), in the order of a group of G threads"""
        vw, nch, G = self._geom(d)
        per = []
        for g in range(G):
            s = 0.0
            for ch in range(g, nch, G):
                s = s + chunk_term(ch * vw, min((ch + 1) * vw, d))
            per.append(s)
        return _group_sum(per)

    def rows_tgrad_dots(self, B, d, rowacc, xs, ys, coefs, accumulate=True):
        self.calls["rows_tgrad_dots"] = self.calls.get("rows_tgrad_dots", 0) + 1
        X = [self._rows(x, B, d).double().tolist() for x in xs]
        Y = [self._rows(y, B, d).double().tolist() for y in ys]
        for r in range(B):
            def term(a, b, r=r):
                s = 0.0
                for x, y, c in zip(X, Y, coefs):
                    dot = 0.0
                    for e in range(a, b):
                        dot = dot + x[r][e] * y[r][e]
                    s = s + c * dot
                return s
            v = self._row_sum(d, term)
            rowacc[r] = float(rowacc[r]) + v if accumulate else v

    def rows_dense_tgrad(self, B, d, erow, g, Ks, times, P, rng, log_d):
        self.calls["rows_dense_tgrad"] = self.calls.get("rows_dense_tgrad", 0) + 1
        nout, nk = g.shape[0], len(Ks)
        theta = torch.zeros(nout, B, dtype=torch.float64)
        dcoef = torch.zeros(nout, B, nk, dtype=torch.float64)
        _lib.check(_lib.load().pn_rows_dense_tgrad_host(B, nout, times.data_ptr(), log_d.data_ptr(), rng.data_ptr(), nk, P,
                                                        theta.data_ptr(), dcoef.data_ptr()))
        K = [self._rows(k, B, d).double().tolist() for k in Ks]
        for r in range(B):
            if not float(log_d[0, r]) > 0.0:
                continue
            for o in range(max(int(rng[0, r]), 0), min(int(rng[1, r]), nout)):
                go = g.detach()[o].reshape(-1)[r * d:(r + 1) * d].double().tolist()
                bp = dcoef[o, r].tolist()

                def term(a, b):
                    s = 0.0
                    for j in range(nk):
                        dot = 0.0
                        for e in range(a, b):
                            dot = dot + go[e] * K[j][r][e]
                        s = s + bp[j] * dot
                    return s
                erow[o, r] = self._row_sum(d, term)

    def rows_tgrad_scatter(self, B, dtrow, rowacc, tbars, coefs, tbar0, c_last, fsal, log_d, hit, rng, erow, times, held, iv, flush=False):
        self.calls["rows_tgrad_scatter"] = self.calls.get("rows_tgrad_scatter", 0) + 1
        opt = lambda x: None if x is None else x.data_ptr()
        for x in list(tbars) + [tbar0]:
            assert x is None or (x.dtype == torch.float64 and x.is_contiguous() and x.numel() == B)
        nt = len(tbars)
        _lib.check(_lib.load().pn_rows_tgrad_scatter_host(
            B, dtrow.shape[0], dtrow.data_ptr(), opt(rowacc), nt, (ctypes.c_void_p * max(nt, 1))(*[x.data_ptr() for x in tbars]),
            (ctypes.c_double * max(nt, 1))(*coefs), opt(tbar0), c_last, 1 if fsal else 0, opt(log_d), opt(hit), opt(rng), opt(erow),
            opt(times), held.data_ptr(), iv.data_ptr(), 1 if flush else 0))

    def rows_tgrad_reduce(self, B, dtrow, dt):
        self.calls["rows_tgrad_reduce"] = self.calls.get("rows_tgrad_reduce", 0) + 1
        nbx = min(max((B + _BLOCK - 1) // _BLOCK, 1), _REDUCE_BLOCKS)
        rows = dtrow.tolist()
        for i, row in enumerate(rows):
            partial = []
            for bx in range(nbx):
                per = []
                for tid in range(_BLOCK):
                    s = 0.0
                    for r in range(bx * _BLOCK + tid, B, nbx * _BLOCK):
                        s = s + row[r]
                    per.append(s)
                partial.append(_block_sum(per))
            lanes = []
            for lane in range(_WAVE):
                t = 0.0
                for bx in range(lane, nbx, _WAVE):
                    t = t + partial[bx]
                lanes.append(t)
            dt[i] = _tree(lanes)
