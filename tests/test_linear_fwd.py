"""The fused forward of func's Linear -> Tanh pairs (pnode_amd/_linearfwd.py): which pairs are eligible, what every other case falls back
to, and that func is left as found.  Host logic: the one place that touches the device, ``pn_linear_fwd``, is stood in for by the torch
expression it replaces, so every fused result must EQUAL the stock modules' and every gradient must be autograd's to round-off."""
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _cpu_vecops import CpuVecOps
from pnode_amd import _funcguard, _linearfwd, options, petsc_adjoint
from problems import MLPFunc, TimeGatedMLPFunc, flat_grads, rel_err


class FwdOps(CpuVecOps):
    """The CPU stand-in with the entry points of pn_linear_fwd: the same shapes, the library expression."""
    fwd_calls = 0

    def linear_fwd_supported(self, rows, out_f, in_f):
        return self.dtype == torch.float32 and rows >= 256 and out_f % 64 == 0 and in_f % 64 == 0

    def linear_fwd(self, x, w, b, tanh, y=None):
        assert self.linear_fwd_supported(x.shape[0], w.shape[0], w.shape[1]) and x.dim() == 2
        FwdOps.fwd_calls += 1
        z = F.linear(x, w, b)
        return torch.tanh(z) if tanh else z


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self):
        self._ops = FwdOps(torch.device("cpu"), torch.float32, 256 * 64)


@pytest.fixture(autouse=True)
def _host_rules(monkeypatch):
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    FwdOps.fwd_calls = 0
    options.clear()
    yield
    options.clear()


def _fwd(f, mode="auto"):
    ode = _Ode()
    fwd = _linearfwd.LinearFwd(ode)
    fwd.install(f, list(f.parameters()), mode)
    return fwd, ode


def _y(d=64, rows=256):
    return torch.randn(rows, d, generator=torch.Generator().manual_seed(1))


def test_the_pairs_of_mlpfunc_run_fused_with_autograds_results():
    f = MLPFunc(64)
    fwd, ode = _fwd(f)
    assert [(type(s), sorted(p)) for s, p in fwd.plans] == [(nn.Sequential, [0, 2, 4])]
    y = _y().requires_grad_(True)
    want = f(0.0, y)
    gw = torch.autograd.grad(want.sum(), [y] + list(f.parameters()))
    assert FwdOps.fwd_calls == 0
    with fwd.window():
        got = f(0.0, y)
    assert FwdOps.fwd_calls == 3 and fwd.n_fused == 3 and fwd.checked and not fwd.disabled
    assert torch.equal(got, want)
    gg = torch.autograd.grad(got.sum(), [y] + list(f.parameters()))
    for a, b in zip(gg, gw):
        assert rel_err(a, b) < 1e-6
    # outside the window func is an ordinary module again
    assert "forward" not in f.net.__dict__
    f(0.0, y)
    assert FwdOps.fwd_calls == 3


class _MyLinear(nn.Linear):
    pass


def _seq_func(*layers):
    class Func(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = nn.Sequential(*layers)

        def forward(self, t, y):
            return self.net(y)
    return Func()


def test_a_linear_subclass_and_a_shared_weight_are_not_fused():
    f = _seq_func(_MyLinear(64, 64), nn.Tanh(), nn.Linear(64, 64))
    fwd, _ = _fwd(f, "1")
    assert fwd.plans == [] and not fwd.active
    a, b = nn.Linear(64, 64), nn.Linear(64, 64)
    b.weight = a.weight
    f = _seq_func(a, nn.Tanh(), b, nn.Tanh(), nn.Linear(64, 64), nn.Tanh())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fwd, _ = _fwd(f, "1")
    assert [sorted(p) for _, p in fwd.plans] == [[4]]
    assert any("shared with another module" in str(c.message) for c in caught)
    with fwd.window():
        f(0.0, _y())
    assert FwdOps.fwd_calls == 1


@pytest.mark.parametrize("where", ["linear", "tanh", "container", "pre", "backward"])
def test_a_user_hook_on_either_module_or_the_container_runs_the_stock_modules(where):
    f = MLPFunc(64)
    fwd, _ = _fwd(f)
    seen = []
    if where == "pre":
        h = f.net[0].register_forward_pre_hook(lambda m, i: seen.append("pre"))
    elif where == "backward":
        h = f.net[1].register_full_backward_hook(lambda m, gi, go: None)
    else:
        m = {"linear": f.net[2], "tanh": f.net[3], "container": f.net}[where]
        h = m.register_forward_hook(lambda m, i, o: seen.append(where))
    y = _y()
    with fwd.window():
        got = f(0.0, y)
    assert FwdOps.fwd_calls == 0 and "forward" not in f.net.__dict__
    assert torch.equal(got, f(0.0, y))
    if where not in ("backward",):
        assert seen
    h.remove()
    with fwd.window():
        f(0.0, y)
    assert FwdOps.fwd_calls == 3


def test_a_forward_that_calls_tanh_itself_has_no_pair():
    class Plain(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.l2 = nn.Linear(64, 64), nn.Linear(64, 64)

        def forward(self, t, y):
            return self.l2(torch.tanh(self.l1(y)))
    fwd, _ = _fwd(Plain())
    assert fwd.plans == [] and not fwd.active


def test_under_autocast_and_for_other_inputs_the_stock_modules_run():
    f = MLPFunc(64)
    fwd, _ = _fwd(f)
    y = _y()
    with fwd.window():
        with torch.autocast("cpu", dtype=torch.bfloat16):
            f(0.0, y)
        assert FwdOps.fwd_calls == 0
        f(0.0, _y(rows=255))                      # outside pn_linear_fwd_supported
        f.double()
        f(0.0, y.double())                        # not the state's fp32
        f.float()
        assert FwdOps.fwd_calls == 0
        f(0.0, _y(rows=512)[::2])                 # not contiguous: the first pair only (its output is)
        assert FwdOps.fwd_calls == 2
        f(0.0, y)
    assert FwdOps.fwd_calls == 5


def test_func_is_left_as_found_when_an_evaluation_raises():
    class Boom(nn.Module):
        def forward(self, x):
            raise ValueError("boom")
    f = _seq_func(nn.Linear(64, 64), nn.Tanh(), Boom())
    fwd, _ = _fwd(f)
    before = _funcguard.snapshot([f])
    with pytest.raises(ValueError, match="boom"):
        with fwd.window():
            f(0.0, _y())
    assert FwdOps.fwd_calls == 1
    assert _funcguard.snapshot([f]) == before and "forward" not in f.net.__dict__


def test_a_failed_forward_check_switches_fusing_off_with_the_reason(monkeypatch):
    f = MLPFunc(64)
    fwd, ode = _fwd(f)
    monkeypatch.setattr(ode._ops, "linear_fwd", lambda x, w, b, tanh, y=None: torch.tanh(F.linear(x, w, b)) + 1e-3)
    y = _y()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with fwd.window():
            got = f(0.0, y)
    assert fwd.disabled and "differ by" in fwd.why and caught
    assert torch.equal(got, f(0.0, y))
    with fwd.window():
        assert "forward" not in f.net.__dict__


def _solve(f, fwd_opt, steps=3):
    options.clear()
    options.set_option("ts_adapt_type", "none")
    if fwd_opt is not None:
        options.set_option("pn_linear_fwd", fwd_opt)
    y0 = _y()
    ode = petsc_adjoint.ODEPetsc(backend=FwdOps)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    for p in f.parameters():
        p.grad = None
    y = y0.clone().requires_grad_(True)
    out = ode.odeint_adjoint(y, torch.tensor([0.0, 0.05 * steps], dtype=torch.float64))
    out[-1].pow(2).sum().backward()
    return out.detach().clone(), y.grad.clone(), flat_grads(f).clone(), ode


def test_a_solve_with_fused_pairs_gives_the_stock_results_and_option_0_runs_stock_modules():
    f = MLPFunc(64, std=0.1)
    o0, y0, p0, ode0 = _solve(f, "0")
    assert ode0._fwd is None and FwdOps.fwd_calls == 0 and ode0.linear_fwd.startswith("stock modules")
    o1, y1, p1, ode1 = _solve(f, None)
    assert ode1._fwd is not None and ode1._fwd.n_fused > 0 and FwdOps.fwd_calls == ode1._fwd.n_fused
    assert ode1.linear_fwd.startswith("fused (3 pairs")
    assert ode1.linear_param_grads.startswith("engine") and ode1._lin.n_autograd == 0 and ode1._lin.n_clean > 0
    assert torch.equal(o0, o1) and rel_err(y1, y0) < 1e-5 and rel_err(p1, p0) < 1e-5
    # ... and with the engine-side sensitivities off the pair's backward returns dW and db to autograd
    options.clear()
    FwdOps.fwd_calls = 0
    f2 = MLPFunc(64, std=0.1)
    options.set_option("ts_adapt_type", "none")
    options.set_option("pn_linear_param_grads", "0")
    y00 = _y()
    ode = petsc_adjoint.ODEPetsc(backend=FwdOps)
    ode.setupTS(y00, f2, step_size=0.05, method="rk4")
    y = y00.clone().requires_grad_(True)
    ode.odeint_adjoint(y, torch.tensor([0.0, 0.15], dtype=torch.float64))[-1].pow(2).sum().backward()
    assert ode._lin is None and ode._fwd.n_fused > 0
    assert rel_err(y.grad, y0) < 1e-5 and rel_err(flat_grads(f2), p0) < 1e-5


@pytest.mark.parametrize("kind", ["late", "upstream", "bias"])
def test_time_gated_func_is_muted_by_clean_exactly_as_before(kind):
    res = {}
    for opt in ("0", "auto"):
        f = TimeGatedMLPFunc(64, std=0.1, kind=kind, gate=0.08)
        o, gy, gp, ode = _solve(f, opt)
        res[opt] = (o, gy, gp, ode._lin.n_autograd, ode._lin.n_clean)
    assert res["auto"][3] == res["0"][3] > 0 and res["auto"][4] == res["0"][4] > 0
    for a, b in zip(res["auto"][:3], res["0"][:3]):
        assert torch.equal(a, b)
    assert FwdOps.fwd_calls == 0                  # (its forward calls the layers one by one: no Sequential.forward, no pair)
