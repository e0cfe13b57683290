"""TEST SCAFFOLDING -- the infinity-norm step control (-ts_adapt_wnormtype infinity): the plain reference of the norm, the bounds
the kernels must meet, the planted operands of tests/test_winf_norm_host.py and tests/test_gpu_winf_norm.py, and the CPU stand-in
with the infinity-norm methods (a subclass of tests/_cpu_rows_tgrad_ops.py, the most derived stand-in).

Bounds (derived, not measured; max is monotone, so a per-term bound is a bound on the norm):
  fp64 states  <= 4 ulp of double, relative: a possibly fused atol + rtol*max, one subtraction, one division.
  fp32 states  <= 1e-6, relative: atol and rtol each rounded to fp32, a product, a sum, a subtraction (not exact when the signs
               differ, class B3 of tests/_wrms_cases.py) and an fp32 division -- at most 8 roundings of 2^-24 = 4.8e-7, doubled.
  a norm whose terms are all exactly zero is exactly 0.0, sign bit clear."""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from pnode_amd import _lib

from _cpu_rows_tgrad_ops import CpuRowsTgradOps

REL = {np.float32: 1e-6, np.float64: 4.0 * 2.0 ** -52}
INF_OPT = (("ts_adapt_wnormtype", "infinity"),)


def winf_ref(un, uh, atol, rtol):
    """max_i |un_i - uh_i| / (atol + rtol max(|un_i|, |uh_i|)) of the two STORED solutions in fp64; NaN if any term is NaN."""
    a, b = np.asarray(un, dtype=np.float64).ravel(), np.asarray(uh, dtype=np.float64).ravel()
    with np.errstate(all="ignore"):
        q = np.abs(a - b) / (atol + rtol * np.maximum(np.abs(a), np.abs(b)))
    return float("nan") if np.isnan(q).any() else float(q.max())


def stored_uhat(un, err):
    with np.errstate(all="ignore"):
        return (un + err).astype(un.dtype)


def meets(T, got, want, what=""):
    """`got` is `want` within the bound of the storage type T; NaN, +inf and an exact zero are matched as such."""
    T = np.dtype(T).type
    if math.isnan(want):
        assert math.isnan(got), (what, got, want)
    elif math.isinf(want):
        assert got == want, (what, got, want)
    elif want == 0.0:
        assert got == 0.0 and not math.copysign(1.0, got) < 0, (what, got)
    else:
        assert abs(got - want) <= REL[T] * want, (what, got, want, abs(got - want) / want)


# ---- planted operands: every term <= 1 but the planted ones
ATOL, RTOL = 1e-3, 1e-3


def background(T, n, seed=0):
    """(un, err) with every term <= 0.5: |un| in [0.5, 2), either sign, |err| <= atol / 2."""
    T = np.dtype(T).type
    g = np.random.default_rng(seed)
    un = ((0.5 + 1.5 * g.random(n)) * np.where(g.random(n) < 0.5, -1.0, 1.0)).astype(T)
    err = (0.5 * ATOL * (2.0 * g.random(n) - 1.0)).astype(T)
    return un, err


def plant(un, err, i, value):
    """Element i becomes un = 1, err such that its term is `value` up to the rounding of err to the storage type."""
    un[i] = 1.0
    err[i] = value * (ATOL + RTOL) / (1.0 - value * RTOL)          # term = err / (atol + rtol (1 + err)) = value


def term_at(un, err, i):
    return winf_ref(un[i:i + 1], stored_uhat(un, err)[i:i + 1], ATOL, RTOL)


def batch_sizes(T):
    """n = 1, one vector minus one element, one workgroup's span - 1 / + 0 / + 1, three workgroups and a ragged tail of 5 (one
    16-byte vector per thread at these sizes: a workgroup spans 256 vectors)."""
    vw = 16 // np.dtype(T).itemsize
    span = 256 * vw
    return [1, vw - 1, span - 1, span, span + 1, 3 * span + 5]


def batch_positions(T, n):
    """Element 0, the last element (the scalar tail where n is ragged), the last element of the last full vector, lane 63 of wave 0,
    lane 0 of the last wave of a workgroup, the first element of the last workgroup -- those that exist at this n."""
    vw = 16 // np.dtype(T).itemsize
    span = 256 * vw
    nvec = n // vw
    last_block = (max(nvec, 1) + 255) // 256 - 1
    pos = [0, n - 1, nvec * vw - 1, 63 * vw, 192 * vw, last_block * span]
    return sorted(set(p for p in pos if 0 <= p < n))


def rows_plant_index(T, d, r):
    """Where row r carries its planted term: its first element, its last element or the last element of its last full chunk."""
    vw = 16 // np.dtype(T).itemsize
    return [0, d - 1, max((d // vw) * vw - 1, 0)][r % 3]


def rows_operands(T, B, d, seed=0):
    """(U, E) of shape [B, d]: row r carries one planted term of r + 2, every other term is <= 0.5."""
    un, err = background(T, B * d, seed)
    U, E = un.reshape(B, d), err.reshape(B, d)
    for r in range(B):
        plant(U[r], E[r], rows_plant_index(T, d, r), r + 2.0)
    return U, E


def rows_ref(U, E):
    return np.array([winf_ref(U[r], stored_uhat(U[r], E[r]), ATOL, RTOL) for r in range(U.shape[0])])


# ---- whole solves
class Cubic(nn.Module):
    """y' = y^3 M, M a rotation plus damping, written element by element (a row's bits do not depend on the batch it is in, on
    any device): an equilibrium at 0, and rows do not mix."""

    def __init__(self):
        super().__init__()
        self.M = nn.Parameter(torch.tensor([[-0.1, 2.0], [-2.0, -0.1]], dtype=torch.float64))

    def forward(self, t, y):
        c, M = y ** 3, self.M
        return torch.stack([c[:, 0] * M[0, 0] + c[:, 1] * M[1, 0], c[:, 0] * M[0, 1] + c[:, 1] * M[1, 1]], dim=1)


class NanFunc(nn.Module):
    def __init__(self):
        super().__init__()
        self.p = nn.Parameter(torch.ones((), dtype=torch.float64))

    def forward(self, t, y):
        return y * self.p * float("nan")


QUIESCENT = torch.tensor([[1.3, -0.4], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)


# ---- the CPU stand-in
def _winf_storage(un, uh, atol, rtol):
    """The norm as the kernels form it: the ratio in the storage type (fp32 states: all of it in fp32), widened, then a max that
    keeps NaN."""
    T = un.dtype.type
    with np.errstate(all="ignore"):
        tol = T(atol) + T(rtol) * np.maximum(np.abs(un), np.abs(uh))
        q = np.abs((un - uh) / tol).astype(np.float64)
    if q.size == 0:
        return 0.0
    return float("nan") if np.isnan(q).any() else float(q.max())


class CpuWinfOps(CpuRowsTgradOps):
    """tests/_cpu_rows_tgrad_ops.py plus what -ts_adapt_wnormtype infinity asks of a backend (pnode_amd/_errnorm.py)."""
    infinity_norm = True

    def combine_winf(self, unew, u, Ks, cb, ce, atol, rtol):
        self.calls["combine_winf"] = self.calls.get("combine_winf", 0) + 1
        n = self.n
        if unew is not None:
            un = self._lin([u] + list(Ks), [1.0] + list(cb))
            self._put(unew, un)
        else:
            un = u[:n]
        err = self._lin(list(Ks), list(ce)) if Ks else torch.zeros(n, dtype=self.dtype)
        uh = (un + err).to(self.dtype)
        self._enorm_inf = _winf_storage(un.detach().numpy(), uh.detach().numpy(), atol, rtol)

    def read_enorm_inf(self):
        return self._enorm_inf

    def rows_combine_winf(self, B, d, unew, u, Ks, cb, ce, h, atol, rtol, enorm):
        self.calls["rows_combine_winf"] = self.calls.get("rows_combine_winf", 0) + 1
        if unew is not None:
            un = self._rlin(B, d, u, Ks, cb, h)
            self._rput(unew, un, B, d)
        else:
            un = self._rows(u, B, d).clone()
        err = self._rlin(B, d, None, Ks, ce, h)
        uh = (un + err).to(self.dtype)
        for r in range(B):
            enorm[r] = _winf_storage(un[r].numpy(), uh[r].numpy(), atol, rtol)

    @property
    def vec_ops_inf(self):
        """The table of `vec_ops` with the combine member pointing at combine_winf."""
        if getattr(self, "_vec_ops_inf", None) is None:
            self.vec_ops                                   # (builds the parent's table and keeps its functions alive)
            at = self._tensor_at

            def combine(st, dt, n, unew, u, nk, K, cb, ce, atol, rtol, work, res):
                try:
                    self.combine_winf(at(unew), at(u), [at(K[j]) for j in range(nk)], [cb[j] for j in range(nk)],
                                      [ce[j] for j in range(nk)], atol, rtol)
                    return 0
                except BaseException as exc:               # surfaces as a failed launch
                    self.loop_error = exc
                    return 1
            f = self._vec_ops_fns
            self._vec_ops_inf_fns = (f[0], _lib.RK_COMBINE_WRMS_FN(combine), f[2], f[3])
            self._vec_ops_inf_struct = _lib.VecOps(*self._vec_ops_inf_fns)
            self._vec_ops_inf = ctypes.cast(ctypes.pointer(self._vec_ops_inf_struct), ctypes.c_void_p)
        return self._vec_ops_inf
