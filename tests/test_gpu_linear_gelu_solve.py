"""-m gpu: whole solves with func's Linear -> GELU pairs owned (pnode_amd/_linearfwd.py, ``-pn_linear_gelu 1``: pn_linear_fwd_pre where
the evaluation is differentiated, pn_linear_fwd with PN_ACT_GELU where it is not, pn_linear_bwd_act reading the saved pre-activation):
Sequential(Linear, GELU, Linear, GELU, Linear) of width 64 on 256 x 64, rk4, 5 steps of 0.05 -- the set-up, method, sizes and margins of
tests/test_gpu_linear_sigmoid_solve.py.

The arithmetic is not torch's bit for bit, so the central statement is accuracy: the fp32 solve with ``-pn_linear_gelu 1`` and the one
without are both measured against the engine's float64 solve (relative 2-norm errors of the solution, dL/dy0 and dL/dtheta); the fused
run's error may be at most MARGIN = 2 times the unfused run's.  Both are round-off walks of the same length over the same operands that
differ in where they round: a norm over 16 384 values of such errors does not move by a factor of two by chance.  GELU is smooth: there
is no kink for an fp32 and an fp64 run to land on opposite sides of.
Measured on MI355X, fused against unfused: solution 1.323e-7 / 1.389e-7 (ratio 0.95), dL/dy0 2.752e-7 / 2.842e-7 (0.97), dL/dtheta
3.135e-7 / 3.063e-7 (1.02)."""
import warnings

import pytest
import torch
import torch.nn as nn

from conftest import require_gpu
from pnode_amd import options, petsc_adjoint
from problems import flat_grads, rel_err

pytestmark = pytest.mark.gpu

MARGIN = 2.0
BASE = dict(ts_adapt_type="none", pn_graph_capture=0)
GELU = dict(BASE, pn_linear_gelu=1)


def _linear(d, g, std):
    lin = nn.Linear(d, d)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(d, d, generator=g, dtype=torch.float64) * std)
        lin.bias.copy_(torch.randn(d, generator=g, dtype=torch.float64) * 0.1)
    return lin


class GeluFunc(nn.Module):
    """Two Linear -> GELU pairs and a bare head (the shape of the KS workload's ODEFunc); weights N(0, std^2), biases N(0, 0.01)."""

    def __init__(self, d=64, seed=0, std=0.3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.net = nn.Sequential(_linear(d, g, std), nn.GELU(), _linear(d, g, std), nn.GELU(), _linear(d, g, std))

    def forward(self, t, y):
        return self.net(y)


class MixedFunc(nn.Module):
    """A ReLU, a Sigmoid, a GELU and a Tanh pair and a bare head."""

    def __init__(self, d=64, seed=0, std=0.3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.net = nn.Sequential(_linear(d, g, std), nn.ReLU(), _linear(d, g, std), nn.Sigmoid(), _linear(d, g, std), nn.GELU(), _linear(d, g, std),
                                 nn.Tanh(), _linear(d, g, std))

    def forward(self, t, y):
        return self.net(y)


def _solve(dev, opts, calls=1, rows=256, d=64, dtype=torch.float32, func=GeluFunc):
    """`calls` training-style calls of one solver; per call (solution, dL/dy0, dL/dtheta); the solver."""
    options.clear()
    for k, v in opts.items():
        options.set_option(k, v)
    f = func(d).to(dtype).to(dev)
    y0 = torch.randn(rows, d, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dtype).to(dev)
    wgt = torch.randn(rows, d, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype).to(dev)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    t = torch.tensor([0.0, 0.25], dtype=torch.float64, device=dev)
    out = []
    for _ in range(calls):
        for p in f.parameters():
            p.grad = None
        y = y0.clone().requires_grad_(True)
        sol = ode.odeint_adjoint(y, t)
        (sol[-1] * wgt).sum().backward()
        torch.cuda.synchronize()
        out.append((sol.detach().clone(), y.grad.clone(), flat_grads(f).clone()))
    options.clear()
    return out, ode


@pytest.fixture(scope="module")
def runs():
    dev = require_gpu()
    ref, _ = _solve(dev, BASE, dtype=torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)        # a self-check that misses says so
        fused, ode_f = _solve(dev, GELU)
    plain, ode_p = _solve(dev, BASE)
    return ref[0], fused[0], plain[0], ode_f, ode_p


def test_the_fused_solve_is_as_close_to_float64_as_the_unfused_one(runs):
    ref, fused, plain, ode_f, ode_p = runs
    assert ode_f._fwd.n_gelu > 0 and ode_p._fwd is None and ode_p.linear_gelu == "off (-pn_linear_gelu 0)"
    for name, r, a, b in zip(("solution", "dL/dy0", "dL/dtheta"), ref, fused, plain):
        assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0
        ef, ep = rel_err(a.double(), r), rel_err(b.double(), r)
        print("%s: fused %.3e  unfused %.3e  ratio %.2f" % (name, ef, ep, ef / ep))
        assert ef <= MARGIN * ep, (name, ef, ep)


def test_statuses_and_counters(runs):
    _, _, _, ode, _ = runs
    fwd = ode._fwd
    assert ode.linear_gelu.startswith("fused (2 pairs") and "refused" not in ode.linear_gelu, ode.linear_gelu
    assert ode.linear_gelu == "fused (2 pairs; %d forward, %d backward calls so far)" % (fwd.n_gelu, fwd.n_gelu_bwd)
    assert fwd.n_gelu > 0 and fwd.n_gelu_bwd > 0 and fwd.n_fused == 0 and fwd.n_fused_bwd == 0 and fwd.n_relu == 0 and fwd.n_bare == 0
    # every evaluation somebody differentiates wrote its pre-activation (on the device the forward sweep keeps its tapes: all of them)
    assert fwd.gelu.n_pre > 0 and fwd.gelu.n_y + fwd.gelu.n_pre == fwd.n_gelu and fwd.n_gelu_bwd >= fwd.gelu.n_pre
    assert fwd.gelu.checked and fwd.gelu.bwd_checked
    assert not (fwd.gelu.disabled or fwd.gelu.bwd_disabled or fwd.sig.disabled or fwd.relu_disabled or fwd.bare_disabled or fwd.disabled or fwd.bwd_disabled)
    assert ode.linear_relu == "off (-pn_linear_relu 0)" and ode.linear_bare == "off (-pn_linear_bare 0)"
    assert ode.linear_sigmoid == "off (-pn_linear_sigmoid 0)"
    assert ode.linear_param_grads.startswith("engine") and ode._lin.n_autograd == 0


def test_graph_replay_equals_eager_launches_bitwise_with_the_gelu_pairs_owned():
    dev = require_gpu()
    eager, _ = _solve(dev, GELU, calls=5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph, ode = _solve(dev, dict(GELU, pn_graph_capture=1), calls=5)
    assert ode.graphs_captured, ode.graph_status
    assert ode._fwd.n_gelu > 0 and ode._fwd.n_gelu_bwd > 0 and not [str(c.message) for c in caught if "hipGraph" in str(c.message)]
    for k, (a, b) in enumerate(zip(graph, eager)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), k


def test_autograds_parameter_sensitivities_with_the_gelu_pairs_owned_equal_the_engines(runs):
    dev = require_gpu()
    _, fused, _, _, _ = runs
    other, ode = _solve(dev, dict(GELU, pn_linear_param_grads=0))
    assert ode._lin is None and ode._fwd.n_gelu > 0 and ode._fwd.n_gelu_bwd > 0
    assert torch.equal(other[0][0], fused[0]) and torch.equal(other[0][1], fused[1])
    assert rel_err(other[0][2], fused[2]) < 1e-5


def test_option_bwd_0_keeps_the_forward_fused_and_runs_gelu_backward_and_matmul(runs):
    dev = require_gpu()
    _, fused, _, _, _ = runs
    other, ode = _solve(dev, dict(GELU, pn_linear_bwd=0))
    assert ode._fwd.n_gelu > 0 and ode._fwd.n_gelu_bwd == 0
    assert torch.equal(other[0][0], fused[0])
    assert rel_err(other[0][1], fused[1]) < 1e-5 and rel_err(other[0][2], fused[2]) < 1e-5


@pytest.mark.parametrize("rows,d", [(128, 64), (256, 104)])
def test_a_shape_outside_pn_linear_fwd_supported_runs_the_stock_modules_bitwise(rows, d):
    """128 rows; width 104, the KS net's, no multiple of 64."""
    dev = require_gpu()
    on, ode = _solve(dev, GELU, rows=rows, d=d)
    off, _ = _solve(dev, BASE, rows=rows, d=d)
    assert ode._fwd is not None and ode._fwd.n_gelu == 0 and ode._fwd.n_gelu_bwd == 0
    assert ode.linear_gelu.startswith("fused (2 pairs; 0 forward, 0 backward"), ode.linear_gelu
    assert "outside pn_linear_fwd_supported" in ode.linear_gelu
    assert all(torch.equal(a, b) for a, b in zip(on[0], off[0]))


def test_a_mixed_net_with_all_five_options_on():
    dev = require_gpu()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        on, ode = _solve(dev, dict(GELU, pn_linear_relu=1, pn_linear_sigmoid=1, pn_linear_bare=1, pn_linear_fwd="auto"), func=MixedFunc)
    off, ode0 = _solve(dev, dict(BASE, pn_linear_fwd=0), func=MixedFunc)
    fwd = ode._fwd
    assert ode0._fwd is None
    assert min(fwd.n_fused, fwd.n_relu, fwd.n_sigmoid, fwd.n_gelu, fwd.n_bare) > 0
    assert min(fwd.n_fused_bwd, fwd.n_relu_bwd, fwd.n_sigmoid_bwd, fwd.n_gelu_bwd, fwd.n_bare_bwd) > 0
    assert fwd.n_fused == fwd.n_relu == fwd.n_sigmoid == fwd.n_gelu == fwd.n_bare and ode._lin.n_autograd == 0
    assert fwd.gelu.n_pre > 0 and fwd.gelu.n_y + fwd.gelu.n_pre == fwd.n_gelu
    assert rel_err(on[0][0], off[0][0]) < 1e-5 and rel_err(on[0][1], off[0][1]) < 1e-5 and rel_err(on[0][2], off[0][2]) < 1e-5
