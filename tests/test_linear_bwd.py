"""The fused backward of func's Linear -> Tanh pairs (pnode_amd/_linearfwd.py, ``-pn_linear_bwd``): when ``_LinearTanh.backward`` takes
``pn_linear_bwd`` and when it keeps the two torch operations.  Host logic: the device entry point is stood in for by the torch expression
it replaces (``tanh_backward`` + ``matmul``), so every fused gradient must EQUAL the unfused one."""
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _cpu_vecops import CpuVecOps
from pnode_amd import _linearfwd, options, petsc_adjoint
from problems import MLPFunc, flat_grads, rel_err


class FwdOnlyOps(CpuVecOps):
    """A backend with pn_linear_fwd's entry points and none for the backward."""
    fwd_calls = 0

    def linear_fwd_supported(self, rows, out_f, in_f):
        return self.dtype == torch.float32 and rows >= 256 and out_f % 64 == 0 and in_f % 64 == 0

    def linear_fwd(self, x, w, b, tanh, y=None):
        FwdOnlyOps.fwd_calls += 1
        z = F.linear(x, w, b)
        return torch.tanh(z) if tanh else z


class BwdOps(FwdOnlyOps):
    """... and with pn_linear_bwd's: the same shapes, the library expression."""
    bwd_calls = 0

    def linear_bwd_supported(self, rows, out_f, in_f):
        return self.dtype == torch.float32 and rows >= 256 and out_f % 64 == 0 and in_f % 64 == 0

    def linear_bwd(self, g, a, w, gz=None, dx=None):
        assert self.linear_bwd_supported(g.shape[0], w.shape[0], w.shape[1]) and g.dim() == 2 and g.shape == a.shape
        assert g.is_contiguous() and a.is_contiguous() and w.is_contiguous()
        BwdOps.bwd_calls += 1
        gz = torch.ops.aten.tanh_backward(g, a)
        return gz, torch.matmul(gz, w)


class OffByAThousandthOps(BwdOps):
    def linear_bwd(self, g, a, w, gz=None, dx=None):
        gz, dx = super().linear_bwd(g, a, w)
        return gz, dx * 1.001


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self, ops=BwdOps):
        self._ops = ops(torch.device("cpu"), torch.float32, 256 * 64)


@pytest.fixture(autouse=True)
def _host_rules(monkeypatch):
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    FwdOnlyOps.fwd_calls = 0
    BwdOps.bwd_calls = 0
    options.clear()
    yield
    options.clear()


def _fwd(f, bwd_mode="auto", ops=BwdOps):
    ode = _Ode(ops)
    fwd = _linearfwd.LinearFwd(ode)
    fwd.install(f, list(f.parameters()), "auto", bwd_mode)
    return fwd, ode


def _y(rows=256, d=64, seed=1):
    return torch.randn(rows, d, generator=torch.Generator().manual_seed(seed))


def _grads(f, fwd, y, loss=lambda out: out.pow(2).sum()):
    with fwd.window():
        out = f(0.0, y)
    wrt = ([y] if y.requires_grad else []) + list(f.parameters())
    return torch.autograd.grad(loss(out), wrt)


def _pair():
    class Func(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = nn.Sequential(nn.Linear(64, 64), nn.Tanh())

        def forward(self, t, y):
            return self.net(y)
    torch.manual_seed(4)
    return Func()


def test_the_backward_of_every_pair_of_mlpfunc_runs_fused_with_the_unfused_gradients():
    f = MLPFunc(64)
    y = _y().requires_grad_(True)
    plain, _ = _fwd(f, "0")
    want = _grads(f, plain, y)
    assert BwdOps.bwd_calls == 0 and plain.n_fused_bwd == 0 and plain.bwd_status.startswith("torch operations")
    fused, _ = _fwd(f)
    got = _grads(f, fused, y)
    assert BwdOps.bwd_calls == 3 and fused.n_fused_bwd == 3 and fused.bwd_checked and not fused.bwd_disabled
    assert fused.bwd_status.startswith("fused (3 calls")
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


def test_an_input_that_needs_no_gradient_keeps_the_torch_operations():
    f = _pair()
    fwd, _ = _fwd(f)
    got = _grads(f, fwd, _y())                     # dW, db only
    assert fwd.n_fused == 1 and BwdOps.bwd_calls == 0 and fwd.n_fused_bwd == 0
    want = torch.autograd.grad(f(0.0, _y()).pow(2).sum(), list(f.parameters()))
    assert all(rel_err(a, b) < 1e-6 for a, b in zip(got, want))


@pytest.mark.parametrize("kind", ["expanded", "transposed"])
def test_a_cotangent_that_is_not_contiguous_keeps_the_torch_operations(kind):
    f = _pair()
    fwd, _ = _fwd(f, "1")
    y = _y().requires_grad_(True)
    loss = (lambda out: out.sum()) if kind == "expanded" else (lambda out: out.t().contiguous().pow(2).sum())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = _grads(f, fwd, y, loss)
    assert fwd.n_fused == 1 and BwdOps.bwd_calls == 0
    assert [c for c in caught if "not contiguous" in str(c.message)]
    want = torch.autograd.grad(loss(f(0.0, y)), [y] + list(f.parameters()))
    assert all(rel_err(a, b) < 1e-6 for a, b in zip(got, want))


def test_an_unsupported_shape_autocast_a_backend_without_the_kernel_and_option_0_keep_the_torch_operations(monkeypatch):
    f = MLPFunc(64)
    y = _y().requires_grad_(True)
    plain, _ = _fwd(f, "0")
    want = _grads(f, plain, y)
    assert plain.n_fused == 3 and BwdOps.bwd_calls == 0
    # outside pn_linear_bwd_supported (the forward's rule still holds)
    fwd, ode = _fwd(f)
    monkeypatch.setattr(ode._ops, "linear_bwd_supported", lambda rows, out_f, in_f: False)
    got = _grads(f, fwd, y)
    assert fwd.n_fused == 3 and BwdOps.bwd_calls == 0 and all(torch.equal(a, b) for a, b in zip(got, want))
    # autocast on while the backward runs
    fwd, _ = _fwd(f)
    with fwd.window():
        out = f(0.0, y)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        torch.autograd.grad(out.pow(2).sum(), [y])
    assert fwd.n_fused == 3 and BwdOps.bwd_calls == 0
    # a backend with linear_fwd only
    fwd, _ = _fwd(f, ops=FwdOnlyOps)
    got = _grads(f, fwd, y)
    assert fwd.n_fused == 3 and BwdOps.bwd_calls == 0 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert "no linear_bwd" in fwd.bwd_status
    # and the fused path on the same operands, for contrast
    fwd, _ = _fwd(f)
    _grads(f, fwd, y)
    assert BwdOps.bwd_calls == 3


def test_option_1_warns_once_with_the_reason():
    f = MLPFunc(64)
    fwd, ode = _fwd(f, "1")
    ode._ops.linear_bwd_supported = lambda rows, out_f, in_f: False
    y = _y().requires_grad_(True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _grads(f, fwd, y)
        _grads(f, fwd, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_bwd 1" in str(c.message)]
    assert len(msgs) == 1 and "outside pn_linear_bwd_supported" in msgs[0]
    assert BwdOps.bwd_calls == 0


def _solve(f, bwd_opt, backend=BwdOps, steps=3, calls=1):
    options.clear()
    options.set_option("ts_adapt_type", "none")
    if bwd_opt is not None:
        options.set_option("pn_linear_bwd", bwd_opt)
    y0 = _y().double().to(next(f.parameters()).dtype)
    ode = petsc_adjoint.ODEPetsc(backend=backend)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    res = []
    for _ in range(calls):
        for p in f.parameters():
            p.grad = None
        y = y0.clone().requires_grad_(True)
        out = ode.odeint_adjoint(y, torch.tensor([0.0, 0.05 * steps], dtype=torch.float64))
        out[-1].pow(2).sum().backward()
        res.append((out.detach().clone(), y.grad.clone(), flat_grads(f).clone()))
    return res, ode


def test_a_whole_solve_with_the_fused_backward_gives_the_gradients_of_option_0():
    f = MLPFunc(64, std=0.1)
    (r0,), ode0 = _solve(f, "0")
    assert BwdOps.bwd_calls == 0 and ode0._fwd.n_fused > 0 and ode0._fwd.n_fused_bwd == 0
    assert ode0.linear_bwd == "torch operations (-pn_linear_bwd 0)"
    (r1,), ode1 = _solve(f, None)
    # rk4 x 3 steps: at least four stage VJPs per step, three pairs each
    n = ode1._fwd.n_fused_bwd
    assert BwdOps.bwd_calls == n and n >= 3 * 4 * 3 and n % 3 == 0
    assert ode1.linear_bwd.startswith("fused (%d calls" % n) and ode1.linear_fwd.startswith("fused (3 pairs")
    assert ode1.linear_param_grads.startswith("engine") and ode1._lin.n_autograd == 0
    assert torch.equal(r0[0], r1[0]) and rel_err(r1[1], r0[1]) < 1e-12 and rel_err(r1[2], r0[2]) < 1e-12


def test_a_failed_backward_check_switches_only_the_backward_off_with_the_reason():
    f = MLPFunc(64, std=0.1)
    (want,), _ = _solve(f, "0")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res, ode = _solve(f, None, backend=OffByAThousandthOps, calls=2)
    msgs = [str(c.message) for c in caught if "backward is switched off" in str(c.message)]
    assert len(msgs) == 1 and "dx by" in msgs[0]
    assert BwdOps.bwd_calls == 1 and ode._fwd.n_fused_bwd == 0 and ode._fwd.bwd_disabled
    assert ode.linear_bwd.startswith("torch operations (pn_linear_bwd and tanh_backward + matmul differ")
    # the forward stays fused, and the gradients are the torch operations' from the failed call on
    assert ode.linear_fwd.startswith("fused (3 pairs") and not ode._fwd.disabled and ode._fwd.n_fused > 0
    for got in res:
        assert torch.equal(got[0], want[0]) and rel_err(got[1], want[1]) < 1e-12 and rel_err(got[2], want[2]) < 1e-12
