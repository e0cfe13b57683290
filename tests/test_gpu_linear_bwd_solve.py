"""-m gpu: whole solves with the backward of func's Linear -> Tanh pairs fused (pnode_amd/_linearfwd.py, pn_linear_bwd): MLPFunc(64) on
256 x 64, rk4 x 5 -- the set-up of tests/test_gpu_linear_fwd_solve.py.

Accuracy: the fp32 solve with the default and the one with ``-pn_linear_bwd 0`` are both measured against the same solve by the engine in
float64 (relative 2-norm errors of dL/dy0 and dL/dtheta); the solutions of the two are equal bit for bit (the forward is untouched) and the
fused run's gradient errors may be at most MARGIN = 2 times the unfused run's: both are round-off walks of the same length over the same
operands that differ in where they round (the split product rounds less than an fp32 chain, 1 - a^2 by an fma or by two operations): a norm
over 16 384 values of such errors does not move by a factor of two by chance.
Measured on MI355X, fused against unfused: dL/dy0 3.486e-7 / 3.719e-7 (ratio 0.94), dL/dtheta 4.314e-7 / 4.485e-7 (0.96)."""
import warnings

import pytest
import torch

from conftest import require_gpu
from pnode_amd import options, petsc_adjoint
from problems import MLPFunc, flat_grads, rel_err

pytestmark = pytest.mark.gpu

MARGIN = 2.0
BASE = dict(ts_adapt_type="none", pn_graph_capture=0)


def _solve(dev, dtype, opts, calls=1, method="rk4", std=0.3):
    """`calls` training-style calls of one solver; per call (solution, dL/dy0, dL/dtheta); the solver."""
    options.clear()
    for k, v in opts.items():
        options.set_option(k, v)
    f = MLPFunc(64, dtype=dtype, std=std).to(dev)
    y0 = torch.randn(256, 64, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(dtype).to(dev)
    wgt = torch.randn(256, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype).to(dev)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, f, step_size=0.05, method=method)
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
    ref, _ = _solve(dev, torch.float64, BASE)
    fused, ode_f = _solve(dev, torch.float32, BASE)
    plain, ode_p = _solve(dev, torch.float32, dict(BASE, pn_linear_bwd=0))
    return ref[0], fused[0], plain[0], ode_f, ode_p


def test_fused_backward_is_as_close_to_float64_as_the_torch_operations(runs):
    ref, fused, plain, ode_f, ode_p = runs
    assert ode_f.linear_bwd.startswith("fused") and ode_f._fwd.n_fused_bwd > 0, ode_f.linear_bwd
    assert ode_f._lin.n_autograd == 0
    assert ode_p.linear_bwd.startswith("torch operations") and ode_p._fwd.n_fused_bwd == 0 and ode_p._fwd.n_fused > 0
    assert torch.equal(fused[0], plain[0])
    for name, r, a, b in list(zip(("solution", "dL/dy0", "dL/dtheta"), ref, fused, plain))[1:]:
        ef, ep = rel_err(a.double(), r), rel_err(b.double(), r)
        print("%s: fused %.3e  unfused %.3e  ratio %.2f" % (name, ef, ep, ef / ep))
        assert ef <= MARGIN * ep, (name, ef, ep)


def test_graph_replay_equals_eager_launches_bitwise_with_the_fused_backward():
    dev = require_gpu()
    eager, _ = _solve(dev, torch.float32, BASE, calls=5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph, ode = _solve(dev, torch.float32, dict(BASE, pn_graph_capture=1), calls=5)
    assert ode.graphs_captured, ode.graph_status
    assert ode._fwd.n_fused_bwd > 0 and not [str(c.message) for c in caught if "hipGraph" in str(c.message)]
    for k, (a, b) in enumerate(zip(graph, eager)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), k


def test_autograds_parameter_sensitivities_with_the_fused_backward_equal_the_default(runs):
    dev = require_gpu()
    _, fused, _, _, _ = runs
    other, ode = _solve(dev, torch.float32, dict(BASE, pn_linear_param_grads=0))
    assert ode._lin is None and ode._fwd.n_fused_bwd > 0
    assert torch.equal(other[0][0], fused[0]) and torch.equal(other[0][1], fused[1])
    assert rel_err(other[0][2], fused[2]) < 1e-5


def test_an_adaptive_dopri5_solve_runs_the_fused_backward_through_per_evaluation_graphs():
    dev = require_gpu()
    opts = dict(ts_adapt_type="basic", pn_graph_capture=1)
    graph, ode = _solve(dev, torch.float32, opts, calls=4, method="dopri5")
    eager, _ = _solve(dev, torch.float32, dict(opts, pn_graph_capture=0), calls=4, method="dopri5")
    assert ode._fwd.n_fused_bwd > 0 and "graph" in ode.graph_status, ode.graph_status
    for a, b in zip(graph, eager):
        assert torch.equal(a[0], b[0]) and rel_err(a[1], b[1]) < 1e-5 and rel_err(a[2], b[2]) < 1e-5
