"""-m gpu: whole solves with func's Linear -> ReLU pairs owned (pnode_amd/_linearfwd.py, ``-pn_linear_relu 1``: pn_linear_fwd with
PN_ACT_RELU, pn_linear_bwd_act): Sequential(Linear, ReLU, Linear, ReLU(inplace), Linear) of width 64 on 256 x 64, rk4, 5 steps of 0.05 --
the set-up of tests/test_gpu_linear_bare_solve.py.

The central statement is bits: the solve with ``-pn_linear_bare 1 -pn_linear_relu 1`` EQUALS the one with ``-pn_linear_bare 1`` in the
solution, dL/dy0 and dL/dtheta.  Forward, the ReLU kernel is relu of the identity kernel; backward, g_z is threshold_backward's and dx is
pn_linear_dx of it; and the same (g_z, x) pairs reach the grouped pn_linear_wgrad in the same order.  A comparison against float64 is
deliberately not made at solve level: an fp32 and an fp64 run can land on opposite sides of a ReLU kink, which moves a gradient by far
more than round-off; tests/test_gpu_linear_relu.py carries the accuracy."""
import warnings

import pytest
import torch
import torch.nn as nn

from conftest import require_gpu
from pnode_amd import options, petsc_adjoint
from problems import flat_grads, rel_err

pytestmark = pytest.mark.gpu

BASE = dict(ts_adapt_type="none", pn_graph_capture=0)
BARE = dict(BASE, pn_linear_bare=1)
RELU = dict(BARE, pn_linear_relu=1)


class ReluFunc(nn.Module):
    """Two Linear -> ReLU pairs, the second ReLU in place, and a bare head; weights N(0, std^2), zero biases, as MLPFunc draws them."""

    def __init__(self, d=64, seed=0, std=0.3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        layers = []
        for k in range(3):
            lin = nn.Linear(d, d)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(d, d, generator=g) * std)
                lin.bias.zero_()
            layers.append(lin)
            if k < 2:
                layers.append(nn.ReLU(inplace=(k == 1)))
        self.net = nn.Sequential(*layers)

    def forward(self, t, y):
        return self.net(y)


def _solve(dev, opts, calls=1, rows=256):
    """`calls` training-style calls of one solver; per call (solution, dL/dy0, dL/dtheta); the solver."""
    options.clear()
    for k, v in opts.items():
        options.set_option(k, v)
    f = ReluFunc().to(dev)
    y0 = torch.randn(rows, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    wgt = torch.randn(rows, 64, generator=torch.Generator().manual_seed(3)).to(dev)
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
    relu, ode_r = _solve(dev, RELU)
    bare, ode_b = _solve(dev, BARE)
    return relu[0], bare[0], ode_r, ode_b


def test_the_solve_with_the_relu_pairs_owned_equals_the_solve_with_every_linear_bare_owned_bitwise(runs):
    relu, bare, _, _ = runs
    for name, a, b in zip(("solution", "dL/dy0", "dL/dtheta"), relu, bare):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
        print("%s: %d of %d values differ, rel. 2-norm %.3e" % (name, int((a != b).sum()), a.numel(), rel_err(a, b)))
        assert torch.equal(a, b), name


def test_statuses_and_counters(runs):
    _, _, ode_r, ode_b = runs
    fwd = ode_r._fwd
    assert ode_r.linear_relu.startswith("fused (2 pairs"), ode_r.linear_relu
    assert fwd.n_relu > 0 and fwd.n_relu_bwd > 0 and fwd.n_fused == 0 and fwd.n_fused_bwd == 0
    assert fwd.relu_checked and fwd.relu_bwd_checked and fwd.bare_checked and fwd.bare_bwd_checked
    assert not (fwd.relu_disabled or fwd.relu_bwd_disabled or fwd.bare_disabled or fwd.bare_bwd_disabled or fwd.disabled or fwd.bwd_disabled)
    assert 2 * fwd.n_bare == fwd.n_relu and 2 * fwd.n_bare_bwd == fwd.n_relu_bwd and ode_r.linear_bare.startswith("fused (1 layers")
    assert ode_r._lin.n_autograd == 0
    assert ode_b.linear_relu == "off (-pn_linear_relu 0)" and ode_b._fwd.n_relu == 0 and ode_b._fwd.n_relu_bwd == 0
    assert ode_b.linear_bare.startswith("fused (3 layers") and ode_b._lin.n_autograd == 0


def test_graph_replay_equals_eager_launches_bitwise_with_the_relu_pairs_owned():
    dev = require_gpu()
    eager, _ = _solve(dev, RELU, calls=5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph, ode = _solve(dev, dict(RELU, pn_graph_capture=1), calls=5)
    assert ode.graphs_captured, ode.graph_status
    assert ode._fwd.n_relu > 0 and ode._fwd.n_relu_bwd > 0 and not [str(c.message) for c in caught if "hipGraph" in str(c.message)]
    for k, (a, b) in enumerate(zip(graph, eager)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), k


def test_autograds_parameter_sensitivities_with_the_relu_pairs_owned_equal_the_engines(runs):
    dev = require_gpu()
    relu, _, _, _ = runs
    other, ode = _solve(dev, dict(RELU, pn_linear_param_grads=0))
    assert ode._lin is None and ode._fwd.n_relu > 0 and ode._fwd.n_relu_bwd > 0
    assert torch.equal(other[0][0], relu[0]) and torch.equal(other[0][1], relu[1])
    assert rel_err(other[0][2], relu[2]) < 1e-5


def test_option_bwd_0_keeps_the_forward_fused_and_runs_threshold_backward_and_matmul(runs):
    dev = require_gpu()
    relu, _, _, _ = runs
    other, ode = _solve(dev, dict(RELU, pn_linear_bwd=0))
    assert ode._fwd.n_relu > 0 and ode._fwd.n_relu_bwd == 0 and ode._fwd.n_bare_bwd == 0
    assert torch.equal(other[0][0], relu[0])
    assert rel_err(other[0][1], relu[1]) < 1e-5 and rel_err(other[0][2], relu[2]) < 1e-5


def test_a_batch_outside_pn_linear_fwd_supported_runs_the_stock_modules_bitwise():
    dev = require_gpu()
    on, ode = _solve(dev, RELU, rows=128)
    off, _ = _solve(dev, BASE, rows=128)
    assert ode._fwd is not None and ode._fwd.n_relu == 0 and ode._fwd.n_relu_bwd == 0 and ode._fwd.n_bare == 0
    assert ode.linear_relu.startswith("fused (2 pairs; 0 forward, 0 backward")
    assert all(torch.equal(a, b) for a, b in zip(on[0], off[0]))
