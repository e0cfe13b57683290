"""-ts_adapt_wnormtype infinity without a GPU: the norm of the CPU stand-in (tests/_winf_cases.py) and the
host finish of the kernels' partials against the plain fp64 reference on the operand regimes of tests/_wrms_cases.py; the option's
plumbing; and whole solves on the stand-in -- quiescent rows that must not loosen the control, the per-sample scope, the gradients
against autograd through the logged steps, and the theta / ARKIMEX steppers.  The kernels themselves: tests/test_gpu_winf_norm.py."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import _winf_cases as wc
import _wrms_cases as rc
from _cpu_vecops import CpuVecOps
from _winf_cases import INF_OPT, Cubic, CpuWinfOps, NanFunc, meets, winf_ref
from pnode_amd import _lib, options, petsc_adjoint
from pnode_amd._lib import PnError

import test_sample_time_grads as stg

CPU = torch.device("cpu")


# ---------------------------------------------------------------------------------------------------- 1. operand regimes
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_stand_in_against_the_reference_on_every_operand_regime(T):
    n = 1027
    ops = CpuWinfOps(CPU, torch.from_numpy(np.zeros(1, dtype=T)).dtype, n)
    for name, un, err, atol, rtol in rc.cases(T, n):
        want = winf_ref(un, wc.stored_uhat(un, err), atol, rtol)
        ops.combine_winf(None, torch.from_numpy(un), [torch.from_numpy(err)], [0.0], [1.0], atol, rtol)
        got = ops.read_enorm_inf()
        assert math.isfinite(got), name                      # class E: finite where the square overflows fp32
        meets(T, got, want, name)
    for name, un, err, atol, rtol in rc.cases(T, n, dyadic=True):
        u, K, exact = rc.write_path_operands(T, un, err)
        unew = torch.empty(n, dtype=ops.dtype)
        ops.combine_winf(unew, torch.from_numpy(u), [torch.from_numpy(k) for k in K], rc.WRITE_CB, rc.WRITE_CE, atol, rtol)
        assert np.array_equal(unew.numpy().view(np.uint8), exact.view(np.uint8)), name
        meets(T, ops.read_enorm_inf(), winf_ref(exact, wc.stored_uhat(exact, err), atol, rtol), name)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_stand_in_rows_find_every_rows_planted_maximum(T):
    for d in (1, 2, 3, 5, 64, 67, 1027):
        for B in (1, 3, 130):
            U, E = wc.rows_operands(T, B, d)
            ops = CpuWinfOps(CPU, torch.from_numpy(U).dtype, B * d)
            enorm = torch.full((B + 4,), -7.0, dtype=torch.float64)
            ops.rows_combine_winf(B, d, None, torch.from_numpy(U.reshape(-1)), [torch.from_numpy(E.reshape(-1))], [0.0], [1.0],
                                  torch.ones(B, dtype=torch.float64), wc.ATOL, wc.RTOL, enorm)
            want = wc.rows_ref(U, E)
            for r in range(B):
                assert abs(want[r] - (r + 2)) <= 1e-5 * (r + 2)                  # the construction: row r's maximum is r + 2
                meets(T, float(enorm[r]), want[r], (d, B, r))
            assert (enorm[B:] == -7.0).all()


# ---------------------------------------------------------------------------------------------------- 4. the host finish
def _finish(partials, n):
    blk = (ctypes.c_double * (len(partials) + 1))(float(len(partials)), *partials)
    v = ctypes.c_double(-1.0)
    _lib.check(_lib.load().pn_winf_finish(blk, n, ctypes.byref(v)))
    return v.value


def test_host_finish_takes_the_largest_partial_and_keeps_nan_inf_and_zero():
    n = 256 * 5
    assert _finish([0.25, 3.0, 0.5, 1.0, 0.0], n) == 3.0
    for at in range(5):
        p = [0.25, 3.0, 0.5, 1.0, 0.125]
        p[at] = float("nan")
        assert math.isnan(_finish(p, n)), at                     # wherever the NaN sits, also before a larger partial
        p[at] = float("inf")
        assert _finish(p, n) == float("inf")
    z = _finish([0.0] * 5, n)
    assert z == 0.0 and math.copysign(1.0, z) > 0
    lib = _lib.load()
    v = ctypes.c_double()
    bad = (ctypes.c_double * 8)(7.0, *([1.0] * 7))               # n = 256 has one workgroup: seven partials cannot be
    assert lib.pn_winf_finish(bad, 256, ctypes.byref(v)) != 0 and b"corrupt block count" in lib.pn_last_error()


# ---------------------------------------------------------------------------------------------------- 5. option plumbing
def _solve(y0, rk="5dp", extra=(), backend=CpuWinfOps, func=None, times=(0.0, 0.3, 0.7), tol=1e-7, grad=True, method="dopri5",
           setup_kw=None, t_grad=False):
    options.clear()
    if rk:
        options.set_option("ts_rk_type", rk)
    options.set_option("ts_rtol", tol)
    options.set_option("ts_atol", tol)
    for k, v in extra:
        options.set_option(k, v)
    try:
        f = Cubic() if func is None else func
        ode = petsc_adjoint.ODEPetsc(backend=backend)
        y = y0.clone().requires_grad_(grad)
        ode.setupTS(y, f, step_size=0.05, method=method, **(setup_kw or {}))
        t = torch.tensor(times, dtype=torch.float64, requires_grad=t_grad)
        pred = ode.odeint_adjoint(y, t)
        out = {"ode": ode, "f": f, "sol": pred.detach().clone(), "log": None if ode._sample else ode.step_log(), "rej": ode.num_rejections}
        if grad:
            w = torch.linspace(0.5, 1.5, pred[0].numel(), dtype=torch.float64).view_as(pred[0])
            sum((pred[i] * w * (1 + 0.1 * i)).sum() for i in range(pred.shape[0])).backward()
            out.update(gu=y.grad.clone(), gp=[p.grad.clone() for p in f.parameters()], gt=t.grad)
        return out
    finally:
        options.clear()


_Y4 = wc.QUIESCENT


def test_wnormtype_2_is_the_option_being_absent_bit_for_bit():
    y0 = torch.tensor([[1.3, -0.4], [0.2, 0.9], [-0.7, 0.1]], dtype=torch.float64)
    a = _solve(y0, t_grad=True)
    b = _solve(y0, extra=(("ts_adapt_wnormtype", "2"),), t_grad=True)
    assert a["log"] == b["log"] and a["rej"] == b["rej"] and len(a["log"]) > 3
    assert torch.equal(a["sol"], b["sol"]) and torch.equal(a["gu"], b["gu"]) and torch.equal(a["gt"], b["gt"])
    assert all(torch.equal(p, q) for p, q in zip(a["gp"], b["gp"]))
    assert not a["ode"]._winf and "combine_winf" not in a["ode"]._ops.calls and a["ode"]._ops.calls["combine_wrms"] > 0


def test_an_unknown_norm_type_is_refused_naming_the_two():
    with pytest.raises(PnError) as e:
        _solve(_Y4, extra=(("ts_adapt_wnormtype", "bogus"),))
    assert "'2'" in str(e.value) and "'infinity'" in str(e.value) and "bogus" in str(e.value)
    assert "-ts_adapt_wnormtype" in str(e.value) and "Implemented: -ts_type" in str(e.value)


def test_a_backend_without_the_capability_is_refused_by_name():
    with pytest.raises(PnError, match="CpuVecOps has no infinity-norm entry points"):
        _solve(_Y4, extra=INF_OPT, backend=CpuVecOps)


def test_ts_view_names_the_norm(capsys):
    _solve(_Y4, extra=INF_OPT + (("ts_view", ""),), grad=False)
    assert "error norm infinity" in capsys.readouterr().out
    _solve(_Y4, extra=(("ts_view", ""),), grad=False)
    assert "error norm 2 (weighted RMS)" in capsys.readouterr().out


@pytest.mark.parametrize("loop", ["native", "python"])
def test_a_func_that_returns_nan_fails_as_it_does_under_the_default_norm(loop):
    seen = []
    for extra in ((), INF_OPT):
        with pytest.raises(Exception) as e:
            _solve(_Y4, extra=extra + (("pn_step_loop", loop),), func=NanFunc(), grad=False)
        seen.append((type(e.value), str(e.value)))
    assert seen[0][0] is seen[1][0] and issubclass(seen[0][0], PnError), seen
    assert seen[0][1] == seen[1][1]


# ---------------------------------------------------------------------------------------------------- 6. quiescent rows
@pytest.mark.parametrize("rk", ["5dp", "3bs"])
@pytest.mark.parametrize("loop", ["native", "python"])
def test_quiescent_rows_do_not_loosen_the_control(rk, loop):
    tol = 1e-8 if rk == "5dp" else 1e-6
    lp = (("pn_step_loop", loop),)
    one = _solve(_Y4[:1], rk, INF_OPT + lp, tol=tol)
    four = _solve(_Y4, rk, INF_OPT + lp, tol=tol)
    assert four["ode"]._winf and four["ode"]._ops.calls["combine_winf"] > 0 and four["ode"]._ops.calls["combine_wrms"] == 0
    assert four["log"] == one["log"] and four["rej"] == one["rej"] and len(one["log"]) > 5
    assert torch.equal(four["sol"][:, 0], one["sol"][:, 0])
    assert (four["sol"][:, 1:] == 0).all()
    # the default norm dilutes the one moving row by sqrt(4): the same pair of solves takes different steps
    one2, four2 = _solve(_Y4[:1], rk, lp, tol=tol), _solve(_Y4, rk, lp, tol=tol)
    assert four2["log"] != one2["log"]


# ---------------------------------------------------------------------------------------------------- 7. sample scope
@pytest.mark.parametrize("rk,mode", [("3bs", "match"), ("5dp", "match"), ("3bs", "interpolate"), ("5dp", "interpolate")])
def test_sample_scope_rows_are_their_batch_of_one_infinity_norm_solves(rk, mode):
    rows = list(range(stg.B))
    full = stg._solve(rk, mode, rows, func="autonomous", extra=INF_OPT, backend=CpuWinfOps)
    ode = full["ode"]
    assert ode._winf and ode._ops.calls["rows_combine_winf"] > 0 and "rows_combine_wrms" not in ode._ops.calls
    for r in rows:
        one = stg._solve(rk, mode, [r], scope="batch", func="autonomous", extra=INF_OPT, backend=CpuWinfOps)["ode"]
        assert ode.sample_step_log(r) == one.step_log(), r
        assert int(ode.sample_steps[r]) == one.num_steps and int(ode.sample_rejections[r]) == one.num_rejections
    assert int(ode.sample_rejections.max()) > 0
    alone = stg._solve(rk, mode, [4], func="autonomous", extra=INF_OPT, backend=CpuWinfOps)         # B = 1 against B = 6, d = 2
    assert torch.equal(alone["sol"][:, 0], full["sol"][:, 4]) and torch.equal(alone["gu"][0], full["gu"][4])


def test_sample_scope_row_does_not_depend_on_its_batch_at_d_67():
    """d = 67: a row spans more than one wave's worth of chunks in fp64 and ends in a ragged chunk."""
    g = torch.Generator().manual_seed(3)
    y0 = torch.randn(5, 67, generator=g, dtype=torch.float64) * torch.tensor([0.2, 0.5, 1.0, 1.5, 2.0], dtype=torch.float64).view(5, 1)

    class F(nn.Module):
        def __init__(self):
            super().__init__()
            self.a = nn.Parameter(torch.tensor(-0.4, dtype=torch.float64))

        def forward(self, t, y):
            return self.a * y ** 3 + 0.3 * torch.roll(y, 1, dims=-1)

    ex = INF_OPT + (("pn_adapt_scope", "sample"),)
    full = _solve(y0, "5dp", ex, func=F(), tol=1e-7, grad=False)
    one = _solve(y0[3:4], "5dp", ex, func=F(), tol=1e-7, grad=False)
    assert torch.equal(one["sol"][:, 0], full["sol"][:, 3])           # (the loss weights of _solve depend on B: no gradient here)
    assert one["ode"].sample_step_log(0) == full["ode"].sample_step_log(3)
    assert len(set(int(s) for s in full["ode"].sample_steps)) > 1


# ---------------------------------------------------------------------------------------------------- 8. gradients
def _autograd_batch(full, rk, mode, rows, func):
    """dL/du0, dL/dtheta and dL/dt of the batch-scope solve by autograd through its logged steps (the restatement of
    tests/test_sample_time_grads.py, which takes any number of rows that share a step log)."""
    f = stg.FUNCS[func]()
    y = stg._y0()[rows].clone().requires_grad_(True)
    t = torch.tensor(stg.TIMES, dtype=torch.float64, requires_grad=True)
    pred = stg._restated_row(f, y, t, full["ode"].step_log(), rk, mode == "interpolate")
    assert stg._rel(pred.detach(), full["sol"]) <= 1e-12
    (pred * stg._weights(len(stg.TIMES))[:, rows]).sum().backward()
    return y.grad, [p.grad for p in f.parameters()], t.grad


@pytest.mark.parametrize("rk,mode", [("5dp", "match"), ("3bs", "interpolate"), ("5dp", "interpolate")])
def test_batch_scope_gradients_equal_autograd_through_the_logged_steps(rk, mode):
    rows = [1, 3, 5]
    full = stg._solve(rk, mode, rows, scope="batch", func="time", extra=INF_OPT, backend=CpuWinfOps)
    assert full["ode"]._winf and full["ode"].num_rejections > 0
    gu, gp, gt = _autograd_batch(full, rk, mode, rows, "time")
    assert stg._rel(full["gu"], gu) <= 1e-12 and stg._rel(full["gt"], gt) <= 1e-12
    for p, q in zip(full["f"].parameters(), gp):
        assert stg._rel(p.grad, q) <= 1e-12


def test_sample_scope_gradients_equal_autograd_through_each_rows_logged_steps():
    rk, mode = "5dp", "interpolate"
    rows = list(range(stg.B))
    full = stg._solve(rk, mode, rows, func="time", extra=INF_OPT, backend=CpuWinfOps)
    ode, w = full["ode"], stg._weights(len(stg.TIMES))
    f = stg.FUNCS["time"]()
    y = stg._y0().clone().requires_grad_(True)
    t = torch.tensor(stg.TIMES, dtype=torch.float64, requires_grad=True)
    loss = 0.0
    for r in rows:
        pred = stg._restated_row(f, y[r:r + 1], t, ode.sample_step_log(r), rk, True)
        assert stg._rel(pred[:, 0].detach(), full["sol"][:, r]) <= 1e-12
        loss = loss + (pred[:, 0] * w[:, r]).sum()
    loss.backward()
    assert stg._rel(full["gu"], y.grad) <= 1e-12 and stg._rel(full["gt"], t.grad) <= 1e-12
    for p, q in zip(full["f"].parameters(), f.parameters()):
        assert stg._rel(p.grad, q.grad) <= 1e-12


# ---------------------------------------------------------------------------------------------------- 9. theta and ARKIMEX
class _Recording(CpuWinfOps):
    """Keeps the pair of solutions of every attempt's estimate and the norm the controller is given."""

    def combine_winf(self, unew, u, Ks, cb, ce, atol, rtol):
        super().combine_winf(unew, u, Ks, cb, ce, atol, rtol)
        assert unew is None and list(ce) == [1.0]
        un = u[: self.n].detach().numpy().copy()
        self.__dict__.setdefault("pairs", []).append((un, (un + Ks[0][: self.n].detach().numpy()).astype(un.dtype), atol, rtol))

    def read_enorm_inf(self):
        v = super().read_enorm_inf()
        self.__dict__.setdefault("given", []).append(v)
        return v


class _Lin(nn.Module):
    def __init__(self, scale):
        super().__init__()
        self.A = nn.Parameter(scale * torch.tensor([[-0.5, 3.0], [-3.0, -0.5]], dtype=torch.float64))

    def forward(self, t, y):
        return y @ self.A


def _check_recorded(ops):
    assert len(ops.given) == len(ops.pairs) > 3
    for v, (un, uh, atol, rtol) in zip(ops.given, ops.pairs):
        meets(np.float64, v, winf_ref(un, uh, atol, rtol))


def test_theta_steps_are_judged_by_the_infinity_norm_of_the_logged_pairs():
    y0 = torch.tensor([[1.0, 0.5], [0.0, 0.0], [0.3, -0.2]], dtype=torch.float64)
    petsc_adjoint._UNPINNED_WARNED.discard("theta_adapt")
    with pytest.warns(petsc_adjoint.PnUnpinnedWarning, match="adaptive beuler / cn steps"):
        out = _solve(y0, None, INF_OPT + (("ts_adapt_type", "basic"),), backend=_Recording, func=_Lin(1.0), times=(0.0, 0.5), tol=1e-5,
                     grad=False, method="cn", setup_kw={"implicit_form": True})
    assert out["ode"]._winf and "combine_wrms" not in [k for k, v in out["ode"]._ops.calls.items() if v]
    _check_recorded(out["ode"]._ops)


def test_arkimex_steps_are_judged_by_the_infinity_norm_of_the_logged_pairs():
    y0 = torch.tensor([[1.0, 0.5], [0.0, 0.0], [0.3, -0.2]], dtype=torch.float64)
    petsc_adjoint._UNPINNED_WARNED.discard("arkimex_adapt")
    with pytest.warns(petsc_adjoint.PnUnpinnedWarning, match="adaptive ARKIMEX steps"):
        out = _solve(y0, None, INF_OPT + (("ts_arkimex_type", "3"),), backend=_Recording, func=_Lin(1.0), times=(0.0, 0.5), tol=1e-6,
                     grad=False, method="imex", setup_kw={"imex_form": True, "func2": _Lin(0.3), "linear_solver": "torch"})
    assert out["ode"]._winf
    _check_recorded(out["ode"]._ops)
