"""-m gpu: whole solves with func's Linear -> Softplus and Linear -> ELU pairs owned (pnode_amd/_linearfwd.py, ``-pn_linear_softplus 1``,
``-pn_linear_elu 1``: pn_linear_fwd with PN_ACT_SOFTPLUS / PN_ACT_ELU, pn_linear_bwd_act): Sequential(Linear, act, Linear, act, Linear) of
width 64 on 256 x 64, rk4, 5 steps of 0.05 -- the set-up of tests/test_gpu_linear_sigmoid_solve.py.

The arithmetic is not torch's bit for bit, so the central statement is accuracy, by that file's method and with its bar: the fp32 solve
with the option on and the one with the stock modules are both measured against the engine's float64 solve (relative 2-norm errors of the
solution, dL/dy0 and dL/dtheta); the fused run's error may be at most MARGIN = 2 times the unfused run's -- the stock modules are the
reference.  Both activations are smooth enough for that: Softplus everywhere; ELU at alpha 1 has a continuous derivative, so an fp32 and
an fp64 run landing on opposite sides of 0 differ by round-off, not by a jump."""
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
KINDS = {"softplus": nn.Softplus, "elu": nn.ELU}


def _on(name, **more):
    return dict(BASE, **dict({"pn_linear_" + name: 1}, **more))


def _linear(d, g, std):
    lin = nn.Linear(d, d)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(d, d, generator=g, dtype=torch.float64) * std)
        lin.bias.copy_(torch.randn(d, generator=g, dtype=torch.float64) * 0.1)
    return lin


def _func(*acts):
    class Func(nn.Module):
        """Linear -> act pairs and a bare head; weights N(0, std^2), biases N(0, 0.01)."""

        def __init__(self, d=64, seed=0, std=0.3):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            layers = []
            for act in acts:
                layers += [_linear(d, g, std), act()]
            self.net = nn.Sequential(*(layers + [_linear(d, g, std)]))

        def forward(self, t, y):
            return self.net(y)
    return Func


FUNCS = {name: _func(cls, cls) for name, cls in KINDS.items()}
MixedFunc = _func(nn.ReLU, nn.Sigmoid, nn.GELU, nn.Softplus, nn.ELU, nn.Tanh)


def _solve(dev, opts, func, calls=1, rows=256, d=64, dtype=torch.float32):
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


_RUNS = {}


def _runs(name):
    if name not in _RUNS:
        dev = require_gpu()
        ref, _ = _solve(dev, BASE, FUNCS[name], dtype=torch.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)        # a self-check that misses says so
            fused, ode_f = _solve(dev, _on(name), FUNCS[name])
        plain, ode_p = _solve(dev, BASE, FUNCS[name])
        _RUNS[name] = (ref[0], fused[0], plain[0], ode_f, ode_p)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(KINDS))
def test_the_fused_solve_is_as_close_to_float64_as_the_solve_with_the_stock_modules(name):
    ref, fused, plain, ode_f, ode_p = _runs(name)
    assert getattr(ode_f._fwd, name).n > 0 and ode_p._fwd is None and getattr(ode_p, "linear_" + name) == "off (-pn_linear_%s 0)" % name
    for what, r, a, b in zip(("solution", "dL/dy0", "dL/dtheta"), ref, fused, plain):
        assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0
        ef, ep = rel_err(a.double(), r), rel_err(b.double(), r)
        print("%s %s: fused %.3e  unfused %.3e  ratio %.2f" % (name, what, ef, ep, ef / ep))
        assert ef <= MARGIN * ep, (name, what, ef, ep)


@pytest.mark.parametrize("name", list(KINDS))
def test_statuses_and_counters(name):
    _, _, _, ode, _ = _runs(name)
    fwd = ode._fwd
    st = getattr(fwd, name)
    other = "elu" if name == "softplus" else "softplus"
    status = getattr(ode, "linear_" + name)
    assert status == "fused (2 pairs; %d forward, %d backward calls so far)" % (st.n, st.n_bwd), status
    assert st.n > 0 and st.n_bwd > 0 and fwd.n_fused == 0 and fwd.n_relu == 0 and fwd.n_sigmoid == 0 and fwd.n_gelu == 0 and fwd.n_bare == 0
    assert st.checked and st.bwd_checked and not st.disabled and not st.bwd_disabled and getattr(fwd, other).n == 0
    assert getattr(ode, "linear_" + other) == "off (-pn_linear_%s 0)" % other and ode.linear_bare == "off (-pn_linear_bare 0)"
    assert ode.linear_param_grads.startswith("engine") and ode._lin.n_autograd == 0


@pytest.mark.parametrize("name", list(KINDS))
def test_graph_replay_equals_eager_launches_bitwise(name):
    dev = require_gpu()
    eager, _ = _solve(dev, _on(name), FUNCS[name], calls=4)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        graph, ode = _solve(dev, _on(name, pn_graph_capture=1), FUNCS[name], calls=4)
    assert ode.graphs_captured, ode.graph_status
    st = getattr(ode._fwd, name)
    assert st.n > 0 and st.n_bwd > 0 and not [str(c.message) for c in caught if "hipGraph" in str(c.message)]
    for k, (a, b) in enumerate(zip(graph, eager)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), k


@pytest.mark.parametrize("name", list(KINDS))
def test_autograds_parameter_sensitivities_equal_the_engines_and_bwd_0_keeps_the_forward(name):
    dev = require_gpu()
    _, fused, _, _, _ = _runs(name)
    other, ode = _solve(dev, _on(name, pn_linear_param_grads=0), FUNCS[name])
    st = getattr(ode._fwd, name)
    assert ode._lin is None and st.n > 0 and st.n_bwd > 0
    assert torch.equal(other[0][0], fused[0]) and torch.equal(other[0][1], fused[1]) and rel_err(other[0][2], fused[2]) < 1e-5
    # -pn_linear_bwd 0: the forward stays fused, the backward runs the torch expression and matmul
    other, ode = _solve(dev, _on(name, pn_linear_bwd=0), FUNCS[name])
    st = getattr(ode._fwd, name)
    assert st.n > 0 and st.n_bwd == 0 and torch.equal(other[0][0], fused[0])
    assert rel_err(other[0][1], fused[1]) < 1e-5 and rel_err(other[0][2], fused[2]) < 1e-5


@pytest.mark.parametrize("name", list(KINDS))
@pytest.mark.parametrize("rows,d", [(128, 64), (256, 104)])
def test_a_shape_outside_pn_linear_fwd_supported_runs_the_stock_modules_bitwise(name, rows, d):
    """128 rows; width 104, no multiple of 64."""
    dev = require_gpu()
    on, ode = _solve(dev, _on(name), FUNCS[name], rows=rows, d=d)
    off, _ = _solve(dev, BASE, FUNCS[name], rows=rows, d=d)
    st = getattr(ode._fwd, name)
    status = getattr(ode, "linear_" + name)
    assert st.n == 0 and st.n_bwd == 0 and status.startswith("fused (2 pairs; 0 forward, 0 backward"), status
    assert "outside pn_linear_fwd_supported" in status
    assert all(torch.equal(a, b) for a, b in zip(on[0], off[0]))


def test_a_mixed_net_with_all_six_pair_options_on():
    dev = require_gpu()
    every = dict(BASE, pn_linear_relu=1, pn_linear_sigmoid=1, pn_linear_gelu=1, pn_linear_softplus=1, pn_linear_elu=1, pn_linear_bare=1,
                 pn_linear_fwd="auto")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        on, ode = _solve(dev, every, MixedFunc)
    off, ode0 = _solve(dev, dict(BASE, pn_linear_fwd=0), MixedFunc)
    fwd = ode._fwd
    assert ode0._fwd is None
    counts = (fwd.n_fused, fwd.n_relu, fwd.n_sigmoid, fwd.n_gelu, fwd.softplus.n, fwd.elu.n, fwd.n_bare)
    assert min(counts) > 0 and len(set(counts)) == 1, counts
    assert min(fwd.n_fused_bwd, fwd.n_relu_bwd, fwd.n_sigmoid_bwd, fwd.n_gelu_bwd, fwd.softplus.n_bwd, fwd.elu.n_bwd, fwd.n_bare_bwd) > 0
    assert ode._lin.n_autograd == 0
    assert rel_err(on[0][0], off[0][0]) < 1e-5 and rel_err(on[0][1], off[0][1]) < 1e-5 and rel_err(on[0][2], off[0][2]) < 1e-5
