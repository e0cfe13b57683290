"""dL/dt of a -pn_adapt_scope sample solve on the CPU stand-in (tests/_cpu_rows_tgrad_ops.py), fp64: row r
is a batch-of-one solve and its dL/dt is section 5.6's rule on its own logged steps; t.grad is the sum over the rows of the [T, B]
matrix `sample_time_grads`.

The problem is the spread cubic spiral of tests/test_sample_adapt.py (six rows of radius 0.05 .. 2, its output times and its
tolerances), autonomous or multiplied by a factor in t that broadcasts against the rows.  The first step size, 0.2, is far too
long for the outer rows: they reject it, the inner rows do not."""
import warnings

import pytest
import torch
import torch.nn as nn

from _cpu_rows_ops import CpuRowsOps
from _cpu_rows_tgrad_ops import CpuRowsTgradOps
from problems import SpiralTruth
from pnode_amd import _lib, options, petsc_adjoint

B = 6
TIMES = [0.0, 0.05, 0.12, 0.2]
TOL = {"3bs": 1e-6, "5dp": 1e-8, "5f": 1e-8, "2a": 1e-4}
STEP = 0.2
CASES = [("3bs", "match"), ("5dp", "match"), ("5f", "match"), ("2a", "match"), ("3bs", "interpolate"), ("5dp", "interpolate")]


class TimeSpiral(nn.Module):
    """The cubic spiral times 1 + 0.5 sin(5 t), plus a drift in t: t enters through tensor operations and broadcasts as (B, 1) or 0-dim."""

    def __init__(self):
        super().__init__()
        self.inner = SpiralTruth()
        self.v = nn.Parameter(torch.tensor([0.3, -0.2], dtype=torch.float64))

    def forward(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype)
        return self.inner(t, y) * (1.0 + 0.5 * torch.sin(5.0 * t)) + self.v * torch.cos(3.0 * t)


FUNCS = {"autonomous": SpiralTruth, "time": TimeSpiral}


def _y0(seed=0):
    g = torch.Generator().manual_seed(seed)
    r = torch.logspace(-1.3, 0.3, B, dtype=torch.float64)
    ang = 6.28 * torch.rand(B, generator=g, dtype=torch.float64)
    return torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=1)


def _weights(T):
    g = torch.Generator().manual_seed(7)
    return torch.rand(T, B, 2, generator=g, dtype=torch.float64) + 0.5


def _solve(rk, mode, rows, scope="sample", func="time", times=TIMES, extra=(), weights=None, backend=CpuRowsTgradOps, backwards=1):
    """Rows `rows` of the spread problem with t.requires_grad; loss = sum(pred * w) with per-row weights (rows do not mix)."""
    options.clear()
    options.set_option("ts_rk_type", rk)
    options.set_option("ts_rtol", TOL[rk])
    options.set_option("ts_atol", TOL[rk])
    options.set_option("pn_adapt_scope", scope)
    options.set_option("pn_output_times", mode)
    for k, v in extra:
        options.set_option(k, v)
    try:
        f = FUNCS[func]()
        ode = petsc_adjoint.ODEPetsc(backend=backend)
        y0 = _y0()
        ode.setupTS(y0[rows], f, step_size=STEP, method="dopri5", enable_adjoint=True)
        w = (_weights(len(times)) if weights is None else weights)[:, rows]
        out = {"ode": ode, "f": f, "gts": []}
        for _ in range(backwards):
            y = y0[rows].clone().requires_grad_(True)
            t = torch.tensor(times, dtype=torch.float64, requires_grad=True)
            pred = ode.odeint_adjoint(y, t)
            (pred * w).sum().backward()
            out["gts"].append(t.grad)
        out.update(sol=pred.detach().clone(), gt=t.grad, gu=y.grad.clone(),
                   dtrow=None if ode.sample_time_grads is None else ode.sample_time_grads.clone())
        return out
    finally:
        options.clear()


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


_ONES = {}


def _batch_of_one(rk, mode, func, r, times=TIMES):
    """t.grad of the -pn_adapt_scope batch solve of row r alone: computed once, shared by the tests that compare against it."""
    key = (rk, mode, func, r, tuple(times))
    if key not in _ONES:
        one = _solve(rk, mode, [r], scope="batch", func=func, times=times)
        _ONES[key] = (one["gt"].clone(), one["ode"].num_steps, one["ode"].num_rejections)
    return _ONES[key]


# ---------------------------------------------------------------------------------------------------- 1. the surface
def test_t_grad_is_a_tensor_and_the_sum_of_the_rows():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        full = _solve("5dp", "match", list(range(B)))
    ode = full["ode"]
    assert isinstance(full["gt"], torch.Tensor) and full["gt"].shape == (len(TIMES),) and full["gt"].dtype == torch.float64
    assert full["dtrow"].shape == (len(TIMES), B) and full["dtrow"].dtype == torch.float64
    assert int(ode.sample_rejections.max()) > 0 and int(ode.sample_rejections.min()) == 0
    assert int(ode.sample_steps.max()) >= 2 * int(ode.sample_steps.min())
    assert float(full["gt"].abs().min()) > 0.0


@pytest.mark.parametrize("rk,mode", CASES)
def test_t_grad_is_the_sum_of_the_rows_in_another_order(rk, mode):
    full = _solve(rk, mode, list(range(B)))
    dtrow = full["dtrow"]
    # the same B numbers per entry, added in two orders: each of the B - 1 additions rounds by at most half an ulp of a partial sum
    bound = (B - 1) * 2.0 ** -53 * dtrow.abs().sum(1)
    assert bool(((full["gt"] - dtrow.sum(1)).abs() <= bound).all()), (full["gt"], dtrow.sum(1))


# ---------------------------------------------------------------------------------------------------- 2. per row against the batch of one
@pytest.mark.parametrize("store", ["0", "1"])
@pytest.mark.parametrize("func", list(FUNCS))
@pytest.mark.parametrize("rk,mode", CASES)
def test_every_column_is_the_batch_of_one_solve_of_that_row(rk, mode, func, store):
    full = _solve(rk, mode, list(range(B)), func=func, extra=(("ts_trajectory_solution_only", store),))
    ode = full["ode"]
    assert int(ode.sample_rejections.max()) > 0
    assert int(ode.sample_steps.max()) >= 2 * int(ode.sample_steps.min()), ode.sample_steps
    worst = 0.0
    for r in range(B):
        gt, steps, rej = _batch_of_one(rk, mode, func, r)
        assert int(ode.sample_steps[r]) == steps and int(ode.sample_rejections[r]) == rej, (r, ode.sample_steps, steps)
        worst = max(worst, _rel(full["dtrow"][:, r], gt))
    print("dL/dt, rows against batch-of-one %s %s %s: steps per row %s, max relative difference %.2e"
          % (rk, mode, func, ode.sample_steps.tolist(), worst))
    assert worst <= 1e-11


# ---------------------------------------------------------------------------------------------------- 3. against autograd
def _restated_row(f, y, t, log, name, dense):
    """An independent fp64 statement of one row as a function of t: the RK steps of the row's logged (t_n, h_n) laid from t[0], every
    step size a constant except the last of each output interval, H = t_i - tau; with interpolated outputs one interval, and the
    extension written in theta = (t_o - tau) / H.  An output exactly on a step end is that step's new state."""
    tab = _lib.get_tableau(name)
    s = tab.s
    A = [[tab.A[i][j] for j in range(s)] for i in range(s)]
    b, c = [tab.b[j] for j in range(s)], [tab.c[j] for j in range(s)]
    P = _lib.get_tableau_dense(name)[1] if dense else None
    T = t.shape[0]
    times = t.tolist()
    rows = [None] * T
    rows[0] = y
    tau = t[0] if T > 1 else torch.zeros((), dtype=torch.float64)
    o = 1 if T > 1 else 0
    N = len(log)
    for k, (tn, h) in enumerate(log):
        if dense or T == 1:
            last, target = k == N - 1, t[T - 1]
        else:
            last, target = abs(tn + h - times[o]) <= 1e-12, t[o]
        H = target - tau if last else torch.tensor(h, dtype=torch.float64)
        K = []
        for i in range(s):
            Yi = y
            for j in range(i):
                if A[i][j] != 0.0:
                    Yi = Yi + (H * A[i][j]) * K[j]
            K.append(f((tau + c[i] * H).view(1, 1), Yi))
        ynew = y
        for j in range(s):
            if b[j] != 0.0:
                ynew = ynew + (H * b[j]) * K[j]
        if dense:
            tend = log[k + 1][0] if k + 1 < N else times[-1]
            while o < T - 1 and times[o] < tend:
                th = (t[o] - tau) / H
                v = y
                for j in range(s):
                    if any(P[j]):
                        v = v + (H * sum(P[j][p] * th ** (p + 1) for p in range(len(P[j])))) * K[j]
                rows[o] = v
                o += 1
            if o < T - 1 and times[o] == tend:
                rows[o] = ynew
                o += 1
        elif last and T > 1:
            rows[o] = ynew
            o += 1
        y, tau = ynew, tau + H
    if dense or T == 1:
        rows[T - 1] = y
    assert all(r is not None for r in rows)
    return torch.stack(rows)


def _check_against_autograd(rk, mode, func="time", times=TIMES, weights=None, landing=None):
    w = _weights(len(times)) if weights is None else weights
    full = _solve(rk, mode, list(range(B)), func=func, times=times, weights=w)
    ode = full["ode"]
    dense = mode == "interpolate" and len(times) > 2
    f = FUNCS[func]()
    y0 = _y0()
    worst = 0.0
    for r in range(B):
        log = ode.sample_step_log(r)
        assert len(log) == int(ode.sample_steps[r])
        t = torch.tensor(times, dtype=torch.float64, requires_grad=True)
        pred = _restated_row(f, y0[r:r + 1], t, log, rk, dense)
        assert _rel(pred[:, 0].detach(), full["sol"][:, r]) <= 1e-12, r
        if landing is not None and r == landing[0]:
            assert torch.equal(pred[landing[1], 0].detach(), full["sol"][landing[1], r])       # a copy of the state, not a polynomial
        (gt,) = torch.autograd.grad((pred[:, 0] * w[:, r]).sum(), t)
        worst = max(worst, _rel(full["dtrow"][:, r], gt))
    print("dL/dt, rows against autograd %s %s %s: max relative difference %.2e" % (rk, mode, func, worst))
    assert worst <= 1e-12
    return ode


@pytest.mark.parametrize("func", list(FUNCS))
@pytest.mark.parametrize("rk,mode", CASES)
def test_every_column_equals_autograd_through_the_rows_logged_steps(rk, mode, func):
    ode = _check_against_autograd(rk, mode, func)
    assert int(ode.sample_rejections.max()) > 0


@pytest.mark.parametrize("rk,mode", CASES)
def test_loss_on_interior_outputs_only(rk, mode):
    w = _weights(len(TIMES))
    w[0] = 0.0
    w[-1] = 0.0
    _check_against_autograd(rk, mode, weights=w)


@pytest.mark.parametrize("rk", ["3bs", "5dp"])
def test_an_output_exactly_on_one_rows_step_end(rk):
    ode = _solve(rk, "interpolate", list(range(B)))["ode"]
    r0 = B - 1
    log = ode.sample_step_log(r0)
    tn, h = log[len(log) // 2]
    t_hit = tn + h
    assert log[len(log) // 2 + 1][0] == t_hit and t_hit not in TIMES
    times = sorted(TIMES + [t_hit])
    again = _check_against_autograd(rk, "interpolate", times=times, landing=(r0, times.index(t_hit)))
    assert [again.sample_step_log(r) for r in range(B)] == [ode.sample_step_log(r) for r in range(B)]


# ---------------------------------------------------------------------------------------------------- 4. independence of the batch
@pytest.mark.parametrize("rk,mode", [("5dp", "match"), ("5dp", "interpolate")])
def test_columns_do_not_depend_on_the_batch_and_a_backward_repeats_its_bits(rk, mode):
    full = _solve(rk, mode, list(range(B)), backwards=2)
    half = _solve(rk, mode, list(range(B // 2, B)))
    assert torch.equal(full["dtrow"][:, B // 2:], half["dtrow"])
    assert torch.equal(full["gts"][0], full["gts"][1])


# ---------------------------------------------------------------------------------------------------- 5. edges
@pytest.mark.parametrize("times", [[0.2], [0.0, 0.2]])
@pytest.mark.parametrize("mode", ["match", "interpolate"])
def test_one_and_two_output_times(times, mode):
    full = _solve("5dp", mode, list(range(B)), times=times)
    assert full["gt"].shape == (len(times),) and full["dtrow"].shape == (len(times), B)
    for r in (0, B - 1):
        gt, steps, _ = _batch_of_one("5dp", mode, "time", r, times)
        assert int(full["ode"].sample_steps[r]) == steps
        assert _rel(full["dtrow"][:, r], gt) <= 1e-11
    _check_against_autograd("5dp", mode, times=times)


def test_reference_defaults_and_a_backend_without_the_entry_points_return_none():
    full = _solve("5dp", "match", list(range(B)), extra=(("pn_reference_defaults", "1"),))
    assert full["gt"] is None and full["gu"] is not None and full["dtrow"] is None
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        plain = _solve("5dp", "match", list(range(B)), backend=CpuRowsOps, backwards=2)
    assert plain["gt"] is None and plain["gu"] is not None and plain["dtrow"] is None
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning) and "pn_adapt_scope" in str(w.message)]) == 1
