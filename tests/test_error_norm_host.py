"""The reference of the weighted RMS error norm, established without a GPU: wrms_ref (tests/_wrms_cases.py: fp64 numpy, exactly
rounded sum, from the two STORED solutions) against the oracle's TSErrorWeightedNorm restatement and against both CPU stand-ins,
on every operand regime the device tests use (tests/test_gpu_error_norm.py), driven the way those drive the kernels.  Building
the cases runs their self-assertions; a wrong class or a wrong reference shows here."""
import numpy as np
import pytest
import torch

import _wrms_cases as wc
from oracle import ts_oracle

NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = [torch.float32, torch.float64]
SIZES = ["VW", "VW+1", 257, 4099]
ROW_DS = [5, 24, 64, 100, 256, 512, 4099]
B = 7


def _n(n, dtype):
    vw = 16 // torch.empty((), dtype=dtype).element_size()
    return {"VW": vw, "VW+1": vw + 1}.get(n, n)


def _agree(got, want):
    return got == want if want == 0.0 else got == pytest.approx(want, rel=1e-14)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_reference_oracle_and_batch_stand_in_agree(dtype, n):
    from _cpu_vecops import CpuVecOps
    n = _n(n, dtype)
    ops = CpuVecOps(torch.device("cpu"), dtype, n)
    for name, un, err, atol, rtol in wc.cases(NP[dtype], n):
        uh = wc.stored_uhat(un, err)
        want = wc.wrms_ref(un, uh, atol, rtol)
        assert np.isfinite(want), name
        assert _agree(ts_oracle.wrms(un, uh, atol, rtol), want), name
        ops.combine_wrms(None, torch.from_numpy(un), [torch.from_numpy(err)], [0.0], [1.0], atol, rtol)
        assert _agree(ops.read_enorm(), want), name
        if name == "all-A1":
            assert want == 0.0 and ops.read_enorm() == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ["VW+1", 4099])
def test_write_path_operands_reproduce_the_case(dtype, n):
    """nk = 3 with dyadic operands: the stand-in writes unew == un bit for bit and its norm is the reference's from the stored
    unew (the construction asserts every partial sum exact)."""
    from _cpu_vecops import CpuVecOps
    n = _n(n, dtype)
    ops = CpuVecOps(torch.device("cpu"), dtype, n)
    for name, un, err, atol, rtol in wc.cases(NP[dtype], n, dyadic=True):
        u, K, ref_unew = wc.write_path_operands(NP[dtype], un, err)
        unew = torch.full((n,), float("nan"), dtype=dtype)
        ops.combine_wrms(unew, torch.from_numpy(u), [torch.from_numpy(k) for k in K], wc.WRITE_CB, wc.WRITE_CE, atol, rtol)
        assert np.array_equal(unew.numpy(), ref_unew) and np.array_equal(ref_unew, un), name
        assert _agree(ops.read_enorm(), wc.wrms_ref(unew.numpy(), wc.stored_uhat(unew.numpy(), err), atol, rtol)), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", ROW_DS)
def test_reference_and_rows_stand_in_agree(dtype, d):
    """Row r is the case vector rotated by r, h = 1."""
    from _cpu_rows_ops import CpuRowsOps
    ops = CpuRowsOps(torch.device("cpu"), dtype, B * d)
    h = torch.ones(B, dtype=torch.float64)
    for name, un, err, atol, rtol in wc.cases(NP[dtype], d):
        U = np.stack([np.roll(un, r) for r in range(B)])
        E = np.stack([np.roll(err, r) for r in range(B)])
        enorm = torch.full((B,), float("nan"), dtype=torch.float64)
        ops.rows_combine_wrms(B, d, None, torch.from_numpy(U.reshape(-1)), [torch.from_numpy(E.reshape(-1))], [0.0], [1.0], h,
                              atol, rtol, enorm)
        for r in range(B):
            assert _agree(float(enorm[r]), wc.wrms_ref(U[r], wc.stored_uhat(U[r], E[r]), atol, rtol)), (name, r)


def test_the_reference_tells_the_regimes_apart():
    """What the norm must not be: with err / tol instead of the stored difference, with |u| alone instead of the maximum, without
    atol -- each moves the reference by far more than any tolerance used on the device, in the class built for it."""
    T, n = np.float32, 257
    named = {name: (un, err, atol, rtol) for name, un, err, atol, rtol in wc.cases(T, n)}

    def variant(un, err, atol, rtol, stored=True, both=True, with_atol=True):
        a, e = un.astype(np.float64), err.astype(np.float64)
        b = wc.stored_uhat(un, err).astype(np.float64) if stored else a + e
        tol = (atol if with_atol else 0.0) + rtol * (np.maximum(np.abs(a), np.abs(b)) if both else np.abs(a))
        return float(np.sqrt(np.mean(((a - b) / tol) ** 2)))
    for name in ("pair0-A1", "pair0-A3", "pair0-A4"):
        c = named[name]
        want = wc.wrms_ref(c[0], wc.stored_uhat(c[0], c[1]), c[2], c[3])
        assert abs(variant(*c, stored=False) - want) > 0.02 * max(want, variant(*c, stored=False)), name   # 2e4 x the fp32 bound
    for name in ("pair0-B1", "pair0-B3", "pair2-B1"):
        c = named[name]
        want = wc.wrms_ref(c[0], wc.stored_uhat(c[0], c[1]), c[2], c[3])
        assert abs(variant(*c, both=False) - want) > 0.2 * want, name
    for name in ("pair0-A2", "pair0-C1", "pair1-mix"):
        c = named[name]
        want = wc.wrms_ref(c[0], wc.stored_uhat(c[0], c[1]), c[2], c[3])
        with np.errstate(divide="ignore", invalid="ignore"):
            assert not abs(variant(*c, with_atol=False) - want) <= 0.01 * want, name
