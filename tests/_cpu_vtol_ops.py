"""TEST SCAFFOLDING -- the CPU stand-in (tests/_winf_cases.py's CpuWinfOps, the most derived one) with the four per-component
entry points of ODEPetsc.setTolerances: ``pn_rk_combine_wrms_v``, ``pn_rk_combine_winf_v``, ``pn_rows_combine_wrms_v`` and
``pn_rows_combine_winf_v``.  Element e is judged against vatol[e % p], vrtol[e % p].  The arithmetic is that of the scalar
stand-ins statement for statement -- the weighted RMS as the oracle's C text forms it (all in double, no contraction, the squares
added in index order), the largest term as _winf_cases._winf_storage does (in the storage type) -- so vectors filled with one
value give the scalar stand-in's bits, and every call is counted by name."""
import math

import numpy as np
import torch

from _winf_cases import CpuWinfOps


def _tile(v, n):
    v = v.detach().numpy().astype(np.float64).ravel()
    assert n % v.size == 0
    return np.tile(v, n // v.size)


def wrms_v(un, uh, atol, rtol):
    """oracle/petsc_ts_restated.c WRMSNorm2 with an (atol, rtol) pair per element: fp64 arrays in, the squares added in index order."""
    u, y = un.astype(np.float64), uh.astype(np.float64)
    with np.errstate(all="ignore"):
        tol = atol + rtol * np.maximum(np.abs(u), np.abs(y))
        e = np.abs(u - y) / tol
        sq = e * e
    s = 0.0
    for x in sq.tolist():
        s += x
    return math.sqrt(s / un.size) if s >= 0.0 else float("nan")


def winf_v(un, uh, atol, rtol):
    """_winf_cases._winf_storage with an (atol, rtol) pair per element, each rounded to the storage type as the kernels do."""
    T = un.dtype.type
    with np.errstate(all="ignore"):
        tol = atol.astype(T) + rtol.astype(T) * np.maximum(np.abs(un), np.abs(uh))
        q = np.abs((un - uh) / tol).astype(np.float64)
    if q.size == 0:
        return 0.0
    return float("nan") if np.isnan(q).any() else float(q.max())


class CpuVtolOps(CpuWinfOps):
    vector_tolerances = True

    def _count(self, what):
        self.calls[what] = self.calls.get(what, 0) + 1

    def _pair(self, unew, u, Ks, cb, ce):
        n = self.n
        if unew is not None:
            un = self._lin([u] + list(Ks), [1.0] + list(cb))
            self._put(unew, un)
        else:
            un = u[:n]
        err = self._lin(list(Ks), list(ce)) if Ks else torch.zeros(n, dtype=self.dtype)
        uh = (un + err).to(self.dtype)
        return un.detach().numpy(), uh.detach().numpy()

    def combine_wrms_v(self, unew, u, Ks, cb, ce, vatol, vrtol):
        self._count("combine_wrms_v")
        un, uh = self._pair(unew, u, Ks, cb, ce)
        self._enorm = wrms_v(un, uh, _tile(vatol, self.n), _tile(vrtol, self.n))

    def combine_winf_v(self, unew, u, Ks, cb, ce, vatol, vrtol):
        self._count("combine_winf_v")
        un, uh = self._pair(unew, u, Ks, cb, ce)
        self._enorm_inf = winf_v(un, uh, _tile(vatol, self.n), _tile(vrtol, self.n))

    def _rows_pair(self, B, d, unew, u, Ks, cb, ce, h):
        if unew is not None:
            un = self._rlin(B, d, u, Ks, cb, h)
            self._rput(unew, un, B, d)
        else:
            un = self._rows(u, B, d).clone()
        err = self._rlin(B, d, None, Ks, ce, h)
        return un, (un + err).to(self.dtype)

    def rows_combine_wrms_v(self, B, d, unew, u, Ks, cb, ce, h, vatol, vrtol, enorm):
        self._count("rows_combine_wrms_v")
        assert vatol.numel() == d and vrtol.numel() == d
        un, uh = self._rows_pair(B, d, unew, u, Ks, cb, ce, h)
        a, r = _tile(vatol, d), _tile(vrtol, d)
        for row in range(B):
            enorm[row] = wrms_v(un[row].numpy(), uh[row].numpy(), a, r)

    def rows_combine_winf_v(self, B, d, unew, u, Ks, cb, ce, h, vatol, vrtol, enorm):
        self._count("rows_combine_winf_v")
        assert vatol.numel() == d and vrtol.numel() == d
        un, uh = self._rows_pair(B, d, unew, u, Ks, cb, ce, h)
        a, r = _tile(vatol, d), _tile(vrtol, d)
        for row in range(B):
            enorm[row] = winf_v(un[row].numpy(), uh[row].numpy(), a, r)
