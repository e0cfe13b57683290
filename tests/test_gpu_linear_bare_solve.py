"""-m gpu: whole solves with func's bare nn.Linear layer owned (pnode_amd/_linearfwd.py, ``-pn_linear_bare 1``: pn_linear_fwd with the
identity, pn_linear_dx): MLPFunc(64) on 256 x 64, rk4 x 5 -- the set-up of tests/test_gpu_linear_bwd_solve.py.

Accuracy: the fp32 solve with ``-pn_linear_bare 1`` and the one with ``0`` are both measured against the same solve by the engine in
float64 (relative 2-norm errors of the solution, dL/dy0 and dL/dtheta); the run with the option on may be at most MARGIN = 2 times as far
off as the run without: both are round-off walks of the same length over the same operands that differ in where they round (the split
product rounds less than an fp32 chain): a norm over 16 384 values of such errors does not move by a factor of two by chance
(tests/test_gpu_linear_bwd_solve.py: the same margin for the same reason).
Measured on MI355X, option 1 against 0: solution 9.900e-8 / 1.007e-7 (ratio 0.98), dL/dy0 3.456e-7 / 3.486e-7 (0.99), dL/dtheta
4.196e-7 / 4.314e-7 (0.97)."""
import warnings

import pytest
import torch

from conftest import require_gpu
from pnode_amd import options, petsc_adjoint
from problems import MLPFunc, flat_grads, rel_err

pytestmark = pytest.mark.gpu

MARGIN = 2.0
BASE = dict(ts_adapt_type="none", pn_graph_capture=0)
BARE = dict(BASE, pn_linear_bare=1)


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
    bare, ode_b = _solve(dev, torch.float32, BARE)
    plain, ode_p = _solve(dev, torch.float32, BASE)
    return ref[0], bare[0], plain[0], ode_b, ode_p


def test_the_owned_bare_layer_is_as_close_to_float64_as_the_library(runs):
    ref, bare, plain, ode_b, ode_p = runs
    fwd = ode_b._fwd
    assert ode_b.linear_bare.startswith("fused (1 layers") and fwd.n_bare > 0 and fwd.n_bare_bwd > 0, ode_b.linear_bare
    assert fwd.bare_checked and fwd.bare_bwd_checked and not fwd.bare_disabled and not fwd.bare_bwd_disabled
    assert 3 * fwd.n_bare == fwd.n_fused and 3 * fwd.n_bare_bwd == fwd.n_fused_bwd
    assert ode_b._lin.n_autograd == 0
    assert ode_p.linear_bare == "off (-pn_linear_bare 0)" and ode_p._fwd.n_bare == 0 and ode_p._fwd.n_bare_bwd == 0 and ode_p._fwd.n_fused > 0
    for name, r, a, b in zip(("solution", "dL/dy0", "dL/dtheta"), ref, bare, plain):
        e1, e0 = rel_err(a.double(), r), rel_err(b.double(), r)
        print("%s: -pn_linear_bare 1 %.3e  0 %.3e  ratio %.2f" % (name, e1, e0, e1 / e0))
        assert e1 <= MARGIN * e0, (name, e1, e0)


def test_graph_replay_equals_eager_launches_bitwise_with_the_bare_layer_owned():
    dev = require_gpu()
    eager, _ = _solve(dev, torch.float32, BARE, calls=5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph, ode = _solve(dev, torch.float32, dict(BARE, pn_graph_capture=1), calls=5)
    assert ode.graphs_captured, ode.graph_status
    assert ode._fwd.n_bare > 0 and ode._fwd.n_bare_bwd > 0 and not [str(c.message) for c in caught if "hipGraph" in str(c.message)]
    for k, (a, b) in enumerate(zip(graph, eager)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), k


def test_an_adaptive_dopri5_solve_runs_the_bare_layer_through_per_evaluation_graphs():
    dev = require_gpu()
    opts = dict(ts_adapt_type="basic", pn_graph_capture=1, pn_linear_bare=1)
    graph, ode = _solve(dev, torch.float32, opts, calls=4, method="dopri5")
    eager, _ = _solve(dev, torch.float32, dict(opts, pn_graph_capture=0), calls=4, method="dopri5")
    assert ode._fwd.n_bare > 0 and ode._fwd.n_bare_bwd > 0 and "graph" in ode.graph_status, ode.graph_status
    for a, b in zip(graph, eager):
        assert torch.equal(a[0], b[0]) and rel_err(a[1], b[1]) < 1e-5 and rel_err(a[2], b[2]) < 1e-5


def test_autograds_parameter_sensitivities_with_the_bare_layer_owned_equal_the_engines(runs):
    dev = require_gpu()
    _, bare, _, _, _ = runs
    other, ode = _solve(dev, torch.float32, dict(BARE, pn_linear_param_grads=0))
    assert ode._lin is None and ode._fwd.n_bare > 0 and ode._fwd.n_bare_bwd > 0
    assert torch.equal(other[0][0], bare[0]) and torch.equal(other[0][1], bare[1])
    assert rel_err(other[0][2], bare[2]) < 1e-5
