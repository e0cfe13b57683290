"""-pn_output_times interpolate (dense output) on the CPU stand-in: the continuous extensions' coefficients, the step sequence
(that of the end points alone), the interpolated values and the discrete adjoint of them against an independent fp64 torch
restatement, the launch / trajectory modes, the number of VJPs, and the refusals."""
import math

import pytest
import torch

from _cpu_dense_ops import CpuDenseOps
from pnode_amd import _lib, options, petsc_adjoint
from pnode_amd._lib import PnError
from problems import MLPFunc, SpiralTruth, TimeDependent

METHODS = {"bosh3": "3bs", "rk4": "4", "dopri5": "5dp"}
CLAIMED_ORDER = {"3bs": 3, "4": 3, "5dp": 4}


def beta(P, j, th):
    return sum(P[j][p] * th ** (p + 1) for p in range(len(P[j])))


# ---------------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("name", ["3bs", "4", "5dp"])
def test_extension_coefficients(name):
    tab = _lib.get_tableau(name)
    order, P = _lib.get_tableau_dense(name)
    assert order == CLAIMED_ORDER[name]
    s = tab.s
    A = [[tab.A[i][j] for j in range(s)] for i in range(s)]
    c = [tab.c[i] for i in range(s)]
    for j in range(s, _lib.PN_MAX_STAGES):
        assert all(v == 0.0 for v in P[j])
    for th in (0.0, 0.1, 0.37, 0.5, 0.81, 1.0):
        bt = [beta(P, j, th) for j in range(s)]
        assert abs(sum(bt) - th) < 1e-14
        # order conditions of the extension, up to its order (trees of order <= 4)
        assert abs(sum(bt[j] * c[j] for j in range(s)) - th ** 2 / 2) < 1e-14
        if order >= 3:
            assert abs(sum(bt[j] * c[j] ** 2 for j in range(s)) - th ** 3 / 3) < 1e-14
            assert abs(sum(bt[i] * A[i][j] * c[j] for i in range(s) for j in range(s)) - th ** 3 / 6) < 1e-14
        if order >= 4:
            assert abs(sum(bt[j] * c[j] ** 3 for j in range(s)) - th ** 4 / 4) < 1e-14
            assert abs(sum(bt[i] * c[i] * A[i][j] * c[j] for i in range(s) for j in range(s)) - th ** 4 / 8) < 1e-14
            assert abs(sum(bt[i] * A[i][j] * c[j] ** 2 for i in range(s) for j in range(s)) - th ** 4 / 12) < 1e-14
            assert abs(sum(bt[i] * A[i][j] * A[j][k] * c[k] for i in range(s) for j in range(s) for k in range(s))
                       - th ** 4 / 24) < 1e-14
    for j in range(s):
        assert abs(beta(P, j, 1.0) - tab.b[j]) < 1e-14


@pytest.mark.parametrize("name,cls", [("3bs", "RK23"), ("5dp", "RK45")])
def test_extension_equals_scipy(name, cls):
    rk = pytest.importorskip("scipy.integrate._ivp.rk")
    Ps = getattr(rk, cls).P
    _, P = _lib.get_tableau_dense(name)
    for j in range(Ps.shape[0]):
        for p in range(Ps.shape[1]):
            assert abs(P[j][p] - float(Ps[j, p])) <= 1e-15 * max(1.0, abs(float(Ps[j, p])))


def test_no_extension_for_other_tableaus():
    for name in ("1fe", "2a", "2b", "3", "5f", "midpoint"):
        with pytest.raises(PnError, match="3bs"):
            _lib.get_tableau_dense(name)


# ---------------------------------------------------------------------------------------------------------------- helpers
def solve(func, y0, t, method, mode="interpolate", adaptive=True, step=0.01, opts=(), grad=True, weights=None):
    options.clear()
    options.set_option("pn_output_times", mode)
    if not adaptive:
        options.set_option("ts_adapt_type", "none")
    for k, v in opts:
        options.set_option(k, v)
    ode = petsc_adjoint.ODEPetsc(backend=CpuDenseOps)
    ode.setupTS(y0.detach(), func, step_size=step, method=method)
    for p in func.parameters():
        p.grad = None
    y0 = y0.detach().clone().requires_grad_(grad)
    y = ode.odeint_adjoint(y0, t)
    out = {"y": y.detach().clone(), "log": ode.step_log(), "ode": ode}
    if grad:
        w = weights if weights is not None else torch.linspace(0.5, 1.5, y.numel(), dtype=y.dtype).view_as(y)
        (y * w).sum().backward()
        out["gy0"] = y0.grad.clone()
        out["gp"] = [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in func.parameters()]
    options.clear()
    return out


def restated(func, y0, times, log, name):
    """An independent fp64 statement: the RK steps of the product's step log and the extension on each step, differentiable."""
    tab = _lib.get_tableau(name)
    _, P = _lib.get_tableau_dense(name)
    s = tab.s
    A = [[tab.A[i][j] for j in range(s)] for i in range(s)]
    b, c = [tab.b[j] for j in range(s)], [tab.c[j] for j in range(s)]
    T = len(times)
    rows = [None] * T
    rows[0] = y0
    y = y0
    o = 1
    for k, (tn, h) in enumerate(log):
        K = []
        for i in range(s):
            Yi = y
            for j in range(i):
                if A[i][j] != 0.0:
                    Yi = Yi + (h * A[i][j]) * K[j]
            K.append(func(tn + c[i] * h, Yi))
        ynew = y
        for j in range(s):
            if b[j] != 0.0:
                ynew = ynew + (h * b[j]) * K[j]
        tend = log[k + 1][0] if k + 1 < len(log) else times[-1]
        while o < T - 1 and times[o] < tend:
            th = (times[o] - tn) / h
            v = y
            for j in range(s):
                cj = h * beta(P, j, th)
                if cj != 0.0:
                    v = v + cj * K[j]
            rows[o] = v
            o += 1
        if o < T - 1 and times[o] == tend:
            rows[o] = ynew
            o += 1
        y = ynew
    rows[T - 1] = y
    assert o == T - 1
    return torch.stack(rows)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- step sequence
@pytest.mark.parametrize("method", ["dopri5", "bosh3"])
@pytest.mark.parametrize("problem", ["spiral", "mlp"])
def test_step_sequence_is_that_of_the_end_points(method, problem):
    if problem == "spiral":
        f, y0, tend = SpiralTruth(), torch.tensor([[2.0, 0.0]], dtype=torch.float64), 4.0
    else:
        f, y0, tend = MLPFunc(d=16, dtype=torch.float64, std=0.5), torch.linspace(-1, 1, 32, dtype=torch.float64).view(2, 16), 2.0
    t = torch.linspace(0.0, tend, 201, dtype=torch.float64)
    a = solve(f, y0, t, method, grad=False)
    e = solve(f, y0, t[[0, -1]], method, grad=False)
    assert a["log"] == e["log"]
    assert a["ode"].num_rejections == e["ode"].num_rejections
    assert torch.equal(a["y"][-1], e["y"][-1])
    assert torch.equal(a["y"][0], y0)
    assert len(a["log"]) < 150
    m = solve(f, y0, t, method, mode="match", grad=False)
    assert len(m["log"]) >= 200


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("method", ["dopri5", "bosh3", "rk4"])
def test_values_against_restatement(method):
    f = SpiralTruth()
    y0 = torch.tensor([[2.0, 0.0]], dtype=torch.float64)
    adaptive = method != "rk4"
    t = torch.linspace(0.0, 1.5 if adaptive else 1.0, 101 if adaptive else 37, dtype=torch.float64)
    ends = solve(f, y0, t[[0, -1]], method, adaptive=adaptive, grad=False)["log"]
    # one output time ON a step end (a copy of that state)
    tl = sorted(set(t.tolist()) | {ends[len(ends) // 2][0]})
    t = torch.tensor(tl, dtype=torch.float64)
    a = solve(f, y0, t, method, adaptive=adaptive, grad=False)
    with torch.no_grad():
        ref = restated(f, y0, t.tolist(), a["log"], METHODS[method])
    assert rel(a["y"], ref) <= 1e-13
    # exact rows: t[0], step ends, t[-1] are the states, bit for bit (the states of the end-points solve)
    e = solve(f, y0, t[[0, -1]], method, adaptive=adaptive, grad=False)
    assert torch.equal(a["y"][-1], e["y"][-1])
    k = tl.index(ends[len(ends) // 2][0])
    # the restatement forms the states in the stand-in's order (u + c_1 K_1 + ...): a state row is that state, bit for bit
    for row in (0, k, len(tl) - 1):
        assert torch.equal(a["y"][row], ref[row]), row


# ---------------------------------------------------------------------------------------------------------------- gradients
def grads_restated(f, y0, t, log, name, w):
    y0r = y0.detach().clone().requires_grad_(True)
    for p in f.parameters():
        p.grad = None
    ref = restated(f, y0r, t.tolist(), log, name)
    (ref * w).sum().backward()
    return y0r.grad.clone(), [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in f.parameters()]


@pytest.mark.parametrize("method", ["bosh3", "rk4", "dopri5"])
def test_gradients_are_the_discrete_adjoint(method):
    f = TimeDependent(3)
    y0 = torch.tensor([[0.5, -0.3, 0.8], [0.1, 0.2, -0.4]], dtype=torch.float64)
    adaptive = method != "rk4"
    if adaptive:
        base = torch.linspace(0.0, 3.0, 61, dtype=torch.float64)
        ends = solve(f, y0, base[[0, -1]], method, grad=False, opts=(("ts_rtol", "1e-3"), ("ts_atol", "1e-3")))["log"]
        assert len(ends) >= 4
        # several outputs in one step, outputs in the first and in the last step, one on a step end
        extra = {ends[0][0] + 0.3 * ends[0][1], ends[0][0] + 0.6 * ends[0][1], ends[-1][0] + 0.4 * ends[-1][1], ends[2][0]}
        t = torch.tensor(sorted(set(base.tolist()) | extra), dtype=torch.float64)
        opts = (("ts_rtol", "1e-3"), ("ts_atol", "1e-3"))
    else:
        t = torch.linspace(0.0, 1.0, 37, dtype=torch.float64)          # off the grid of h = 0.01 (some land on it)
        opts = ()
    w = torch.randn((t.numel(),) + tuple(y0.shape), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    a = solve(f, y0, t, method, adaptive=adaptive, opts=opts, weights=w)
    gy0, gp = grads_restated(f, y0, t, a["log"], METHODS[method], w)
    assert rel(a["gy0"], gy0) <= 1e-10
    assert len(a["gp"]) == len(gp)
    for x, r in zip(a["gp"], gp):
        assert torch.equal(x, r) or rel(x, r) <= 1e-10


# ---------------------------------------------------------------------------------------------------------------- modes
MODES = [
    (("pn_step_loop", "python"),),
    (("ts_trajectory_solution_only", "0"),),
    (("ts_trajectory_solution_only", "1"),),
    (("ts_trajectory_max_cps_ram", "3"),),
    (("ts_trajectory_solution_only", "0"), ("pn_trajectory_retain_graph", "0")),
    (("ts_trajectory_solution_only", "0"), ("pn_trajectory_retain_graph", "1")),
]


@pytest.mark.parametrize("method", ["dopri5", "rk4"])
def test_same_bits_in_every_mode(method):
    """Step loop, checkpoint and tape modes: the same bits, for each way of forming the nn.Linear sensitivities.  Between those
    two ways (-pn_linear_param_grads auto: one accumulating GEMM alpha*G^T x into mu; 0: autograd's G^T x, then mu += alpha*dW)
    the project guarantees the outputs and dL/dy0 bit for bit and dL/dtheta to round-off (tests/test_linear_param_grads.py):
    the BLAS rounds the two GEMM forms differently on some CPUs."""
    f = MLPFunc(d=8, dtype=torch.float64, std=0.5)
    y0 = torch.linspace(-1, 1, 24, dtype=torch.float64).view(3, 8)
    adaptive = method != "rk4"
    t = torch.linspace(0.0, 1.0, 41, dtype=torch.float64)
    step = 0.01 if adaptive else 0.03
    bases = {}
    for lin in ("auto", "0"):
        base = bases[lin] = solve(f, y0, t, method, adaptive=adaptive, step=step, opts=(("pn_linear_param_grads", lin),))
        assert base["ode"].linear_param_grads.startswith("engine" if lin == "auto" else "autograd")
        assert len(base["log"]) > 3
        for opts in MODES:
            opts = opts + (("pn_linear_param_grads", lin),)
            o = solve(f, y0, t, method, adaptive=adaptive, step=step, opts=opts)
            assert o["log"] == base["log"], opts
            assert torch.equal(o["y"], base["y"]), opts
            assert torch.equal(o["gy0"], base["gy0"]), opts
            for x, r in zip(o["gp"], base["gp"]):
                assert torch.equal(x, r), opts
    a, b = bases["auto"], bases["0"]
    assert a["log"] == b["log"]
    assert torch.equal(a["y"], b["y"])
    assert torch.equal(a["gy0"], b["gy0"])
    for x, r in zip(a["gp"], b["gp"]):
        assert torch.equal(x, r) or rel(x, r) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- VJP count
@pytest.mark.parametrize("method", ["dopri5", "bosh3", "rk4"])
def test_vjp_count(method):
    f = SpiralTruth()
    y0 = torch.tensor([[2.0, 0.0]], dtype=torch.float64)
    adaptive = method != "rk4"
    opts = (("pn_trajectory_retain_graph", "0"), ("ts_trajectory_solution_only", "0"))
    t_end = 1.0
    e = solve(f, y0, torch.tensor([0.0, t_end], dtype=torch.float64), method, adaptive=adaptive, opts=opts)
    n_end = e["ode"].nfe_backward
    tl, hl = e["log"][-1]
    inside_last = torch.tensor([0.0, 0.25, 0.5, tl + 0.5 * hl, t_end], dtype=torch.float64)
    a = solve(f, y0, inside_last, method, adaptive=adaptive, opts=opts)
    assert a["log"] == e["log"]
    fsal = method != "rk4"
    assert a["ode"].nfe_backward == n_end + (1 if fsal else 0)
    t0, h0 = e["log"][0]
    not_last = torch.tensor([0.0, t0 + 0.5 * h0, t_end], dtype=torch.float64)
    if len(e["log"]) > 1:
        b = solve(f, y0, not_last, method, adaptive=adaptive, opts=opts)
        assert b["ode"].nfe_backward == n_end


# ---------------------------------------------------------------------------------------------------------------- refusals
def _setup(method="dopri5", **kw):
    ode = petsc_adjoint.ODEPetsc(backend=CpuDenseOps)
    ode.setupTS(torch.zeros(1, 2, dtype=torch.float64), SpiralTruth(), method=method, **kw)
    return ode


def test_refusals():
    options.clear()
    try:
        options.set_option("pn_output_times", "nearest")
        with pytest.raises(PnError, match="match or interpolate"):
            _setup()
        options.clear()
        options.set_option("pn_output_times", "interpolate")
        for method in ("euler", "rk2", "midpoint"):
            with pytest.raises(PnError, match="5dp"):
                _setup(method)
        for rk in ("2a", "3", "5f"):
            options.set_option("ts_rk_type", rk)
            with pytest.raises(PnError, match="5dp"):
                _setup()
        options.clear()
        options.set_option("pn_output_times", "interpolate")
        with pytest.raises(PnError, match="theta / IMEX"):
            _setup("cn", implicit_form=True)
        ode = _setup()
        t = torch.linspace(0, 1, 5, dtype=torch.float64)
        ode.odeint(torch.tensor([[2.0, 0.0]], dtype=torch.float64), t)
        ode._begin_adjoint(torch.zeros(2, dtype=torch.float64))
        with pytest.raises(PnError, match="interpolate"):
            ode.petsc_adjointsolve(t, 2)
        with pytest.raises(PnError, match="strictly increasing"):
            ode.odeint(torch.tensor([[2.0, 0.0]], dtype=torch.float64), torch.tensor([0.0, 0.5, 0.5, 1.0], dtype=torch.float64))
    finally:
        options.clear()


def test_match_is_the_default_and_view_names_the_mode(capsys):
    options.clear()
    try:
        options.set_option("ts_view", "")
        ode = _setup()
        ode.odeint(torch.tensor([[2.0, 0.0]], dtype=torch.float64), torch.linspace(0, 1, 5, dtype=torch.float64))
        assert "output times: match" in capsys.readouterr().out
        options.set_option("pn_output_times", "interpolate")
        ode = _setup()
        ode.odeint(torch.tensor([[2.0, 0.0]], dtype=torch.float64), torch.linspace(0, 1, 5, dtype=torch.float64))
        assert "output times: interpolate" in capsys.readouterr().out
    finally:
        options.clear()
