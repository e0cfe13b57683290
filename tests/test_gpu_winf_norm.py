"""-m gpu: the infinity-norm kernels (pn_combine_winf_kernel in csrc/pn_kernels.hip, pn_rows_combine_winf_kernel in csrc/pn_rows.hip,
winf_term<T> / nan_max in csrc/pn_device.h) against the plain fp64 reference of tests/_winf_cases.py, with its derived bounds.

 1. every operand regime of tests/_wrms_cases.py, both forms (the writing one with unew bit-equal to the exact result), aligned
    bases and bases one element off;
 2. one planted maximum among terms <= 1/2 at the seams of the launch geometry: a reduction that loses a lane, a wave, a
    workgroup or the ragged tail cannot pass;
 3. the rows kernel with a different planted maximum in every row: a wrong shuffle width or an LDS mix-up moves a row's maximum
    into its neighbour; dead rows, the canary behind enorm, a row alone against the row in a batch, rows against the batch kernel;
 4. NaN, +inf and zero through every level of both trees;
 5. whole solves on the device: quiescent rows, a func that returns NaN."""
import math

import numpy as np
import pytest
import torch

import _winf_cases as wc
import _wrms_cases as rc
from _winf_cases import INF_OPT, meets, winf_ref
from conftest import require_gpu
from pnode_amd import options, petsc_adjoint
from pnode_amd._lib import PnError
from pnode_amd._vecops import HipVecOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
NP = {torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(autouse=True)
def _gpu():
    require_gpu()


def _dev(arr, off=0):
    """A host array on the device, `off` elements into an allocation of its own (off = 1: not 16-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    v = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)[off:]
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _norm(ops, un, err, off=0, atol=wc.ATOL, rtol=wc.RTOL):
    ops.combine_winf(None, _dev(un, off), [_dev(err, off)], [0.0], [1.0], atol, rtol)
    return ops.read_enorm_inf()


# ----------------------------------------------------------------------------------------------------- 1. regimes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("write", [False, True])
def test_regimes_batch_kernel(dtype, n, off, write):
    T = NP[dtype]
    ops = HipVecOps(DEV, dtype, n)
    for name, un, err, atol, rtol in rc.cases(T, n, dyadic=write):
        if write:
            u0, K0, exact = rc.write_path_operands(T, un, err)
            unew = torch.full((n + off,), float("nan"), dtype=dtype, device=DEV)[off:]
            ops.combine_winf(unew, _dev(u0, off), [_dev(k, off) for k in K0], rc.WRITE_CB, rc.WRITE_CE, atol, rtol)
            got = ops.read_enorm_inf()
            assert np.array_equal(_bits(unew), _bits(torch.from_numpy(exact))), name
            un = exact
        else:
            got = _norm(ops, un, err, off, atol, rtol)
        want = winf_ref(un, wc.stored_uhat(un, err), atol, rtol)
        print("%s: got %.17g want %.17g" % (name, got, want))
        assert math.isfinite(got), name                          # class E: finite in fp32, where the square overflows
        meets(T, got, want, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [5, 64, 100, 4099])
@pytest.mark.parametrize("write", [False, True])
def test_regimes_rows_kernel(dtype, d, write):
    """B = 7, row r is the case vector rotated by r; where d is a whole number of chunks the scalar form, one element off, too."""
    T, B = NP[dtype], 7
    ops = HipVecOps(DEV, dtype, B * d)
    h = torch.ones(B, dtype=torch.float64, device=DEV)
    roll = lambda x: np.stack([np.roll(x, r) for r in range(B)])
    for name, un, err, atol, rtol in rc.cases(T, d, dyadic=write):
        U, E = roll(un), roll(err)
        for off in (0, 1):
            enorm = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
            if write:
                u0, K0, exact = rc.write_path_operands(T, un, err)
                unew = torch.full((B * d + off,), float("nan"), dtype=dtype, device=DEV)[off:]
                ops.rows_combine_winf(B, d, unew, _dev(roll(u0).reshape(-1), off), [_dev(roll(k).reshape(-1), off) for k in K0],
                                      rc.WRITE_CB, rc.WRITE_CE, h, atol, rtol, enorm)
                assert np.array_equal(_bits(unew.view(B, d)), _bits(torch.from_numpy(roll(exact)))), name
                U = roll(exact)
            else:
                ops.rows_combine_winf(B, d, None, _dev(U.reshape(-1), off), [_dev(E.reshape(-1), off)], [0.0], [1.0], h, atol, rtol, enorm)
            got = enorm.tolist()
            for r in range(B):
                assert math.isfinite(got[r])
                meets(T, got[r], winf_ref(U[r], wc.stored_uhat(U[r], E[r]), atol, rtol), (name, off, r))


# ----------------------------------------------------------------------------------------------------- 2. planted maximum
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off", [0, 1])
def test_planted_maximum_batch_kernel(dtype, off):
    T = NP[dtype]
    for n in wc.batch_sizes(T):
        ops = HipVecOps(DEV, dtype, n)
        base_un, base_err = wc.background(T, n, seed=n)
        assert winf_ref(base_un, wc.stored_uhat(base_un, base_err), wc.ATOL, wc.RTOL) <= 0.5
        for p in wc.batch_positions(T, n):
            un, err = base_un.copy(), base_err.copy()
            wc.plant(un, err, p, 3.0)
            want = wc.term_at(un, err, p)
            assert abs(want - 3.0) <= 1e-5 and want == winf_ref(un, wc.stored_uhat(un, err), wc.ATOL, wc.RTOL)
            got = _norm(ops, un, err, off)
            print("n %d position %d: got %.17g want %.17g" % (n, p, got, want))
            meets(T, got, want, (n, p))


# ----------------------------------------------------------------------------------------------------- 3. planted maxima, rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 2, 3, 5, 64, 67, 1027, 65544])
def test_planted_maxima_rows_kernel(dtype, d):
    T = NP[dtype]
    U, E = wc.rows_operands(T, 130, d, seed=d)
    want = wc.rows_ref(U, E)
    assert all(abs(want[r] - (r + 2)) <= 1e-5 * (r + 2) for r in range(130))          # the construction: row r's maximum is r + 2
    inside = None
    for B in (130, 3, 1):
        ops = HipVecOps(DEV, dtype, B * d)
        h = torch.ones(B, dtype=torch.float64, device=DEV)
        enorm = torch.full((B + 8,), -7.0, dtype=torch.float64, device=DEV)
        u, e = _dev(U[:B].reshape(-1)), _dev(E[:B].reshape(-1))
        ops.rows_combine_winf(B, d, None, u, [e], [0.0], [1.0], h, wc.ATOL, wc.RTOL, enorm)
        got = enorm.tolist()
        for r in range(B):
            meets(T, got[r], want[r], (d, B, r))
        assert got[B:] == [-7.0] * 8                                                # the canary behind enorm[B - 1]
        if B == 130:
            inside = enorm[:130].clone()
            for r in (1, 64, 129):                                                  # a row alone: the bits it has inside B = 130
                one = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
                HipVecOps(DEV, dtype, d).rows_combine_winf(1, d, None, _dev(U[r]), [_dev(E[r])], [0.0], [1.0], h[:1], wc.ATOL, wc.RTOL, one)
                assert np.array_equal(_bits(one), _bits(inside[r:r + 1])), (d, r)
        else:
            assert np.array_equal(_bits(enorm[:B]), _bits(inside[:B])), (d, B)
        ops.combine_winf(None, u, [e], [0.0], [1.0], wc.ATOL, wc.RTOL)             # the batch kernel over the flattened [B, d]
        flat = ops.read_enorm_inf()
        assert flat == max(got[:B]) and flat == got[B - 1], (d, B)


# ----------------------------------------------------------------------------------------------------- 4. NaN, +inf, zero
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_inf_and_zero_batch_kernel(dtype):
    T = NP[dtype]
    for n in wc.batch_sizes(T):
        ops = HipVecOps(DEV, dtype, n)
        base_un, base_err = wc.background(T, n, seed=n)
        for off in (0, 1):
            z = _norm(ops, base_un, np.zeros_like(base_err), off)
            assert z == 0.0 and math.copysign(1.0, z) > 0, (n, off)
            for p in wc.batch_positions(T, n):
                un, err = base_un.copy(), base_err.copy()
                wc.plant(un, err, (p + 1) % n, 3.0)                  # a larger finite term beside it must not hide the NaN
                err[p] = np.nan
                assert math.isnan(_norm(ops, un, err, off)), (n, off, p)
                un[p] = np.nan                                       # in the state itself
                assert math.isnan(_norm(ops, un, base_err, off)), (n, off, p)
                un, err = base_un.copy(), base_err.copy()
                un[p], err[p] = 0.0, np.finfo(T).max / 2             # finite operands, rtol = 0: the ratio itself overflows to +inf
                assert _norm(ops, un, err, off, wc.ATOL, 0.0) == float("inf"), (n, off, p)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 3, 64, 67, 1027, 65544])
def test_nan_inf_and_zero_rows_kernel(dtype, d):
    T, B = NP[dtype], 5
    U, E = wc.rows_operands(T, B, d, seed=d)
    ops = HipVecOps(DEV, dtype, B * d)
    h = torch.ones(B, dtype=torch.float64, device=DEV)

    def run(U, E, rtol=wc.RTOL):
        enorm = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
        ops.rows_combine_winf(B, d, None, _dev(U.reshape(-1)), [_dev(E.reshape(-1))], [0.0], [1.0], h, wc.ATOL, rtol, enorm)
        return enorm.tolist()
    clean = run(U, E)
    z = run(U, np.zeros_like(E))
    assert z == [0.0] * B and all(math.copysign(1.0, v) > 0 for v in z)
    for r in (0, 2, 4):
        for p in sorted({0, d - 1, d // 2, wc.rows_plant_index(T, d, r + 1)}):
            E2 = E.copy()
            E2[r, p] = np.nan
            got = run(U, E2)
            assert math.isnan(got[r]) and got[:r] + got[r + 1:] == clean[:r] + clean[r + 1:], (d, r, p, got)
            U2 = U.copy()
            U2[r, p], E2[r, p] = 0.0, np.finfo(T).max / 2             # finite operands, rtol = 0: the ratio itself overflows to +inf
            got = run(U2, E2, 0.0)
            assert got[r] == float("inf") and all(math.isfinite(v) for v in got[:r] + got[r + 1:]), (d, r, p, got)


# ----------------------------------------------------------------------------------------------------- 5. whole solves
def _solve(y0, rk, extra=(), func=None, tol=1e-8, times=(0.0, 0.3, 0.7)):
    options.clear()
    options.set_option("ts_rk_type", rk)
    options.set_option("ts_rtol", tol)
    options.set_option("ts_atol", tol)
    for k, v in extra:
        options.set_option(k, v)
    try:
        f = (wc.Cubic() if func is None else func).to(DEV)
        ode = petsc_adjoint.ODEPetsc()
        y = y0.to(DEV)
        ode.setupTS(y, f, step_size=0.05, method="dopri5")
        with torch.no_grad():
            sol = ode.odeint_adjoint(y, torch.tensor(times, dtype=torch.float64, device=DEV))
        torch.cuda.synchronize()
        return {"ode": ode, "sol": sol.cpu(), "log": ode.step_log(), "rej": ode.num_rejections}
    finally:
        options.clear()


@pytest.mark.parametrize("rk", ["5dp", "3bs"])
@pytest.mark.parametrize("loop", ["native", "python"])
def test_quiescent_rows_do_not_loosen_the_control(rk, loop):
    tol = 1e-8 if rk == "5dp" else 1e-6
    lp = (("pn_step_loop", loop),)
    one = _solve(wc.QUIESCENT[:1], rk, INF_OPT + lp, tol=tol)
    four = _solve(wc.QUIESCENT, rk, INF_OPT + lp, tol=tol)
    assert four["ode"]._winf and four["log"] == one["log"] and four["rej"] == one["rej"] and len(one["log"]) > 5
    assert torch.equal(four["sol"][:, 0], one["sol"][:, 0]) and (four["sol"][:, 1:] == 0).all()
    one2, four2 = _solve(wc.QUIESCENT[:1], rk, lp, tol=tol), _solve(wc.QUIESCENT, rk, lp, tol=tol)
    assert four2["log"] != one2["log"]


def test_a_func_that_returns_nan_fails_as_it_does_under_the_default_norm():
    seen = []
    for extra in ((), INF_OPT, INF_OPT + (("pn_adapt_scope", "sample"),)):
        with pytest.raises(Exception) as e:
            _solve(wc.QUIESCENT, "5dp", extra, func=wc.NanFunc())
        seen.append(type(e.value))
    assert seen[0] is seen[1] is seen[2] and issubclass(seen[0], PnError), seen
