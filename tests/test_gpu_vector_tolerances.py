"""-m gpu: the per-component error-norm kernels (pn_combine_wrms_v_kernel / pn_combine_winf_v_kernel in csrc/pn_kernels.hip,
pn_rows_combine_v_kernel in csrc/pn_rows.hip) behind ODEPetsc.setTolerances.

 1. exact: vectors filled with one value give the scalar entry point's norm bit for bit and the same unew bytes, at every size at
    which the launch takes another path (one vector per thread and four, the ragged tail, bases one element off);
 2. exact: the power-of-two rescaling identity, kernels and whole solves;
 3. non-constant vectors against the float64 numpy statement of tests/_vtol_cases.py at the sizes and periods at which the index
    can go wrong, on operands whose fused chains are exact.  The bars are those the scalar counterparts are held to:
      weighted RMS, batch   rel 1e-6 (fp32) / 1e-9 (fp64)                  tests/test_gpu_kernels.py::test_combine_wrms
      weighted RMS, rows    rtol 1e-6 (fp32) / 1e-9 (fp64), atol 1e-12     tests/test_gpu_sample_adapt.py::test_rows_combine_wrms
      largest term, both    tests/_winf_cases.py meets(): rel 1e-6 (fp32) / 4 ulp (fp64)   tests/test_gpu_winf_norm.py
      unew on exact chains  bit equality                                   tests/test_gpu_winf_norm.py (its writing form)
 4. NaN in one element (rows: in one row only), guard elements around unew and enorm, the period vectors only read;
 5. whole solves on the device: constant vectors against the scalar solve, and ROBER's scales."""
import math

import numpy as np
import pytest
import torch

import _vtol_cases as vc
from _winf_cases import meets
from conftest import require_gpu
from pnode_amd._vecops import HipVecOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
NORMS = ["2", "infinity"]
NP = {torch.float32: np.float32, torch.float64: np.float64}
WRMS_REL = {np.float32: 1e-6, np.float64: 1e-9}
GUARD = 8                                   # elements on either side of unew (32 or 64 bytes: the view stays 16-byte aligned)
BIG = 3 * 2 ** 20                           # four vectors per thread in both dtypes; 1024 % 3 and 512 % 3 are not zero


@pytest.fixture(autouse=True)
def _gpu():
    require_gpu()


def _dev(arr, off=0):
    t = torch.from_numpy(np.ascontiguousarray(arr))
    v = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)[off:]
    v.copy_(t)
    return v


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _guarded(n, dtype, off=0):
    """(whole allocation, the n-element view GUARD + off elements in): sentinel -77 everywhere."""
    whole = torch.full((n + 2 * GUARD + off,), -77.0, dtype=dtype, device=DEV)
    return whole, whole[GUARD + off: GUARD + off + n]


def _guards_intact(whole, n, off=0):
    w = whole.cpu()
    return bool((w[: GUARD + off] == -77.0).all()) and bool((w[GUARD + off + n:] == -77.0).all())


def _batch(ops, norm, unew, u, K, cb, ce, a, r):
    """The norm by the scalar entry point (a, r floats) or the _v one (tensors)."""
    vec = isinstance(a, torch.Tensor)
    if norm == "2":
        (ops.combine_wrms_v if vec else ops.combine_wrms)(unew, u, K, cb, ce, a, r)
        return ops.read_enorm()
    (ops.combine_winf_v if vec else ops.combine_winf)(unew, u, K, cb, ce, a, r)
    return ops.read_enorm_inf()


def _rows(ops, norm, B, d, unew, u, K, cb, ce, h, a, r, enorm):
    vec = isinstance(a, torch.Tensor)
    name = "rows_combine_" + ("wrms" if norm == "2" else "winf") + ("_v" if vec else "")
    getattr(ops, name)(B, d, unew, u, K, cb, ce, h, a, r, enorm)


# ---------------------------------------------------------------------------------------------------- 1. constant vectors
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
def test_constant_vectors_are_the_scalar_batch_kernel_bit_for_bit(dtype, norm):
    atol, rtol = 3e-4, 7e-4
    for n, p, nk, off in ((1, 1, 1, 0), (7, 7, 7, 0), (1000, 1, 6, 0), (4099, 4099, 7, 0), (4099, 1, 3, 1), (4098, 3, 7, 0),
                          (4096, 512, 7, 0), (4096 * 512, 512, 7, 0), (BIG, 3, 2, 0), (BIG + 3, BIG + 3, 1, 0)):
        g = torch.Generator().manual_seed(n + nk)
        u, *K = [torch.randn(n + off, generator=g, dtype=dtype).to(DEV)[off:] for _ in range(nk + 1)]
        cb = [0.01 * (j + 1) for j in range(nk)]
        ce = [1e-4 * (-1) ** j * (j + 1) for j in range(nk)]
        ops = HipVecOps(DEV, dtype, n)
        va, vr = torch.full((p,), atol, dtype=torch.float64, device=DEV), torch.full((p,), rtol, dtype=torch.float64, device=DEV)
        for write in (False, True):
            x = torch.full((n + off,), float("nan"), dtype=dtype, device=DEV)[off:] if write else None
            y = torch.full((n + off,), float("nan"), dtype=dtype, device=DEV)[off:] if write else None
            want = _batch(ops, norm, x, u, K, cb, ce, atol, rtol)
            got = _batch(ops, norm, y, u, K, cb, ce, va, vr)
            assert got == want and want > 0, (n, p, nk, off, write, got, want)
            if write:
                assert np.array_equal(_bits(x), _bits(y)), (n, p, nk, off)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
def test_constant_vectors_are_the_scalar_rows_kernel_bit_for_bit(dtype, norm):
    atol, rtol = 3e-4, 7e-4
    for B, d, nk, off in ((1, 3, 1, 0), (5, 7, 7, 0), (64, 64, 7, 0), (5, 130, 3, 0), (64, 64, 2, 1), (3, 1028, 7, 0)):
        g = torch.Generator().manual_seed(B * d + nk)
        u, *K = [torch.randn(B * d + off, generator=g, dtype=dtype).to(DEV)[off:] for _ in range(nk + 1)]
        cb = [0.01 * (j + 1) for j in range(nk)]
        ce = [1e-4 * (-1) ** j * (j + 1) for j in range(nk)]
        h = (0.5 + torch.rand(B, generator=g, dtype=torch.float64)).to(DEV)
        ops = HipVecOps(DEV, dtype, B * d)
        va, vr = torch.full((d,), atol, dtype=torch.float64, device=DEV), torch.full((d,), rtol, dtype=torch.float64, device=DEV)
        for write in (False, True):
            x = torch.full((B * d + off,), float("nan"), dtype=dtype, device=DEV)[off:] if write else None
            y = torch.full((B * d + off,), float("nan"), dtype=dtype, device=DEV)[off:] if write else None
            e1, e2 = torch.full((B,), -7.0, dtype=torch.float64, device=DEV), torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
            _rows(ops, norm, B, d, x, u, K, cb, ce, h, atol, rtol, e1)
            _rows(ops, norm, B, d, y, u, K, cb, ce, h, va, vr, e2)
            assert np.array_equal(_bits(e1), _bits(e2)) and bool((e1 > 0).all()), (B, d, nk, off, write)
            if write:
                assert np.array_equal(_bits(x), _bits(y)), (B, d, nk, off)


# ---------------------------------------------------------------------------------------------------- 2. power-of-two rescaling
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
def test_power_of_two_rescaling_kernels(dtype, norm):
    """The _v kernel on (u, K) under atol_e = s_e a against the scalar kernel on (u / s, K / s) under a: the same norm, unew == s v."""
    T, a, rtol = NP[dtype], 1e-3, 1e-3
    for B, nk in ((1, 1), (6, 7), (1366, 7), (2 ** 20, 3)):
        n, d = 3 * B, 3
        g = np.random.default_rng(B)
        u = ((0.5 + 1.5 * g.random(n)) * np.where(g.random(n) < 0.5, -1.0, 1.0)).astype(T)
        K = [(2.0 * g.random(n) - 1.0).astype(T) for _ in range(nk)]
        cb = [0.05 * (j + 1) / nk for j in range(nk)]
        ce = [2e-3 * (-1.0) ** j * (j + 1) / nk for j in range(nk)]
        s = np.tile(np.array(vc.SCALES, dtype=T), B)
        va = torch.tensor(a * np.array(vc.SCALES), dtype=torch.float64, device=DEV)
        vr = torch.full((d,), rtol, dtype=torch.float64, device=DEV)
        ops = HipVecOps(DEV, dtype, n)
        x, y = torch.empty(n, dtype=dtype, device=DEV), torch.empty(n, dtype=dtype, device=DEV)
        got = _batch(ops, norm, x, _dev(u), [_dev(k) for k in K], cb, ce, va, vr)
        want = _batch(ops, norm, y, _dev(u / s), [_dev(k / s) for k in K], cb, ce, a, rtol)
        assert got == want and want > 0, (B, nk, got, want)
        assert np.array_equal(_bits(x), _bits(y * _dev(s))), (B, nk)
        if B <= 1366:                                             # rows: every row of d = 3 against its scaled twin
            h = torch.ones(B, dtype=torch.float64, device=DEV)
            e1, e2 = torch.empty(B, dtype=torch.float64, device=DEV), torch.empty(B, dtype=torch.float64, device=DEV)
            _rows(ops, norm, B, d, x, _dev(u), [_dev(k) for k in K], cb, ce, h, va, vr, e1)
            _rows(ops, norm, B, d, y, _dev(u / s), [_dev(k / s) for k in K], cb, ce, h, a, rtol, e2)
            assert np.array_equal(_bits(e1), _bits(e2)) and np.array_equal(_bits(x), _bits(y * _dev(s))), (B, nk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("scope", ["batch", "sample"])
def test_power_of_two_rescaling_solves(scope, norm, dtype):
    a, rtol = 1e-6, 1e-6
    s = torch.tensor(vc.SCALES, dtype=dtype)
    y0 = vc.y0_mix(dtype)
    kw = dict(grad=False, device=DEV, step_size=0.5)
    big = vc.solve(y0, vc.Mix(dtype), "5dp", scope, norm, tol=(rtol, 1e-2), vtol=(None, (a * s.double()).to(DEV)), **kw)
    small = vc.solve(y0 / s, vc.Mix(dtype, vc.SCALES), "5dp", scope, norm, tol=(rtol, a), **kw)
    assert big["log"] == small["log"] and big["counts"] == small["counts"]
    assert torch.equal(big["sol"], small["sol"] * s)
    assert (sum(big["counts"][1]) if scope == "sample" else big["counts"][1]) > 0
    assert big["status"].startswith("vector (period 3 of n 15")


# ---------------------------------------------------------------------------------------------------- 3. against float64 numpy
BATCH_CASES = sorted(set((n, p) for n in (1, 3, 7, 1000, 4099) for p in (1, 3, n) if n % p == 0))
BATCH_CASES += [(4098, 3), (4096, 512), (BIG, 3), (BIG, BIG // 8)]       # ... and four vectors per thread, where the index hops thrice


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
def test_batch_kernels_against_the_float64_statement(dtype, norm):
    T = NP[dtype]
    for n, p in BATCH_CASES:
        va, vr = vc.period_vectors(p, seed=n + p)
        dva, dvr = _dev(va), _dev(vr)
        ta, tr = np.tile(va, n // p), np.tile(vr, n // p)
        ops = HipVecOps(DEV, dtype, n)
        for nk in ((1, 7) if n < BIG else (2,)):
            u, K, cb, ce = vc.operands(T, n, nk, seed=n + nk)
            for write in (False, True):
                for off in ((0, 1) if n in (7, 4099) else (0,)):
                    whole, unew = _guarded(n, dtype, off) if write else (None, None)
                    got = _batch(ops, norm, unew, _dev(u, off), [_dev(k, off) for k in K], cb, ce, dva, dvr)
                    un, uh = vc.exact_pair(u, K, cb, ce, write)
                    what = (n, p, nk, write, off)
                    if write:
                        assert np.array_equal(_bits(unew), _bits(torch.from_numpy(un.astype(T)))), what
                        assert _guards_intact(whole, n, off), what
                    if norm == "2":
                        want = vc.wrms_ref(un, uh, ta, tr)
                        print("wrms", what, "got %.17g want %.17g" % (got, want))
                        assert got == pytest.approx(want, rel=WRMS_REL[T]), what
                    else:
                        want = vc.winf_ref(un, uh, ta, tr)
                        print("winf", what, "got %.17g want %.17g" % (got, want))
                        meets(T, got, want, what)
        assert np.array_equal(dva.cpu().numpy(), va) and np.array_equal(dvr.cpu().numpy(), vr), (n, p)      # only read


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
def test_rows_kernels_against_the_float64_statement(dtype, norm):
    T = NP[dtype]
    for B in (1, 5, 64):
        for d in (3, 7, 64, 130):
            va, vr = vc.period_vectors(d, seed=B + d)
            dva, dvr = _dev(va), _dev(vr)
            ops = HipVecOps(DEV, dtype, B * d)
            hh = np.array([(0.5, 1.0, 2.0)[r % 3] for r in range(B)])
            h = _dev(hh)
            for nk in (1, 7):
                u, K, cb, ce = vc.operands(T, B * d, nk, seed=B * d + nk)
                for write in (False, True):
                    for off in ((0, 1) if d == 64 else (0,)):
                        whole, unew = _guarded(B * d, dtype, off) if write else (None, None)
                        enorm = torch.full((B + 8,), -7.0, dtype=torch.float64, device=DEV)
                        _rows(ops, norm, B, d, unew, _dev(u, off), [_dev(k, off) for k in K], cb, ce, h, dva, dvr, enorm[4: 4 + B])
                        un, uh = vc.exact_pair(u.reshape(B, d), [k.reshape(B, d) for k in K], cb, ce, write, hh)
                        what = (B, d, nk, write, off)
                        got = enorm.tolist()
                        assert got[:4] == [-7.0] * 4 and got[4 + B:] == [-7.0] * 4, what                   # the guards of enorm
                        if write:
                            assert np.array_equal(_bits(unew), _bits(torch.from_numpy(un.astype(T).reshape(-1)))), what
                            assert _guards_intact(whole, B * d, off), what
                        if norm == "2":
                            want = torch.tensor([vc.wrms_ref(un[r], uh[r], va, vr) for r in range(B)], dtype=torch.float64)
                            assert torch.allclose(torch.tensor(got[4: 4 + B], dtype=torch.float64), want, rtol=WRMS_REL[T], atol=1e-12), what
                        else:
                            for r in range(B):
                                meets(T, got[4 + r], vc.winf_ref(un[r], uh[r], va, vr), what + (r,))
            assert np.array_equal(dva.cpu().numpy(), va) and np.array_equal(dvr.cpu().numpy(), vr), (B, d)  # only read


# ---------------------------------------------------------------------------------------------------- 4. NaN
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
def test_a_nan_propagates_as_in_the_scalar_kernels(dtype, norm):
    T = NP[dtype]
    for n, p in ((7, 7), (4098, 3), (BIG, 3)):
        u, K, cb, ce = vc.operands(T, n, 2, seed=n)
        va, vr = vc.period_vectors(p, seed=n)
        ops = HipVecOps(DEV, dtype, n)
        for at in sorted({0, n - 1, n // 2, (n // 4) * 4 - 1}):
            K2 = [k.copy() for k in K]
            K2[1][at] = np.nan
            got = _batch(ops, norm, None, _dev(u), [_dev(k) for k in K2], cb, ce, _dev(va), _dev(vr))
            want = _batch(ops, norm, None, _dev(u), [_dev(k) for k in K2], cb, ce, 1e-3, 1e-3)
            assert math.isnan(got) and math.isnan(want), (n, p, at, got, want)
    B, d = 5, 130
    u, K, cb, ce = vc.operands(T, B * d, 2, seed=1)
    va, vr = vc.period_vectors(d, seed=2)
    ops = HipVecOps(DEV, dtype, B * d)
    h = torch.ones(B, dtype=torch.float64, device=DEV)

    def run(K, a, r):
        enorm = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
        _rows(ops, norm, B, d, None, _dev(u), [_dev(k) for k in K], cb, ce, h, a, r, enorm)
        return enorm.tolist()
    clean = run(K, _dev(va), _dev(vr))
    for r in (0, 2, 4):
        for c in (0, d - 1, d // 2):
            K2 = [k.copy() for k in K]
            K2[0][r * d + c] = np.nan
            got, scalar = run(K2, _dev(va), _dev(vr)), run(K2, 1e-3, 1e-3)
            assert math.isnan(got[r]) and got[:r] + got[r + 1:] == clean[:r] + clean[r + 1:], (r, c, got)
            assert [math.isnan(v) for v in got] == [math.isnan(v) for v in scalar]


def test_the_entry_points_refuse_a_period_that_does_not_fit():
    from pnode_amd._lib import PnError
    ops = HipVecOps(DEV, torch.float64, 12)
    u, k = torch.ones(12, dtype=torch.float64, device=DEV), torch.ones(12, dtype=torch.float64, device=DEV)
    v5, v4 = torch.full((5,), 1e-3, dtype=torch.float64, device=DEV), torch.full((4,), 1e-3, dtype=torch.float64, device=DEV)
    with pytest.raises(PnError, match="pn_rk_combine_wrms_v: the period must divide n"):
        ops.combine_wrms_v(None, u, [k], [0.0], [1.0], v5, v5)
    with pytest.raises(PnError, match="pn_rk_combine_winf_v: the period must divide n"):
        ops.combine_winf_v(None, u, [k], [0.0], [1.0], v5, v5)
    e, h = torch.zeros(4, dtype=torch.float64, device=DEV), torch.ones(4, dtype=torch.float64, device=DEV)
    with pytest.raises(PnError, match="pn_rows_combine_wrms_v: the period must be d"):
        ops.rows_combine_wrms_v(4, 3, None, u, [k], [0.0], [1.0], h, v4, v4, e)
    with pytest.raises(PnError, match="pn_rows_combine_winf_v: the period must be d"):
        ops.rows_combine_winf_v(4, 3, None, u, [k], [0.0], [1.0], h, v4, v4, e)


# ---------------------------------------------------------------------------------------------------- 5. whole solves
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("scope", ["batch", "sample"])
@pytest.mark.parametrize("rk", ["3bs", "5dp"])
def test_solves_with_constant_vectors_are_the_scalar_solves(rk, scope, norm, dtype):
    y0, tol = vc.y0_mix(dtype), {"5dp": 1e-6, "3bs": 1e-4}[rk]
    scalar = vc.solve(y0, vc.Mix(dtype), rk, scope, norm, tol=(tol, tol), device=DEV, step_size=0.5)
    c = lambda shape: torch.full(shape, tol, dtype=torch.float64, device=DEV)
    vec = vc.solve(y0, vc.Mix(dtype), rk, scope, norm, tol=(1e-2, 1e-2), vtol=(c((3,)), c((3,) if scope == "sample" else (5, 3))),
                   device=DEV, step_size=0.5)
    assert scalar["status"].startswith("scalar") and vec["status"].startswith("vector (period %d of n 15" % (3 if scope == "sample" else 15))
    vc.same_solve(scalar, vec)
    assert (sum(scalar["counts"][1]) if scope == "sample" else scalar["counts"][1]) > 0


def test_robers_scales_on_the_device():
    B = 8
    y0 = torch.zeros(B, 3, dtype=torch.float64)
    y0[:, 0] = torch.linspace(0.9, 1.1, B, dtype=torch.float64)
    steps = []
    for atol in (1e-8, torch.tensor([1e-8, 1e-12, 1e-8], dtype=torch.float64, device=DEV), 1e-12):
        out = vc.solve(y0, vc.Rober(), "5dp", tol=(1e-6, 1e-8), vtol=(1e-6, atol), times=(0.0, 0.01), grad=False, step_size=1e-5, device=DEV)
        steps.append(out["counts"][0])
    print("accepted steps: scalar 1e-8 %d, vector %d, scalar 1e-12 %d" % tuple(steps))
    assert steps[0] < steps[1] < steps[2]
