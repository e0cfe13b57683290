"""func's nn.Linear -> nn.ReLU pairs (pnode_amd/_linearfwd.py, ``-pn_linear_relu 0|1``): which children are such a pair, that the default
changes nothing, what every other case falls back to, the self-checks of their own, and the C entry point's refusals.  Host logic:
``pn_linear_fwd`` with ``PN_ACT_RELU`` and ``pn_linear_bwd_act`` are stood in for by the torch expressions they replace
(``relu(F.linear)``; ``threshold_backward`` and ``matmul``), so every output must EQUAL the stock modules' and every gradient agrees
with autograd's to 1e-6 in the relative 2-norm (one sum formed by ``mm`` here and by ``addmm`` / ``linear_backward`` there: the bar of
tests/test_linear_bare.py)."""
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _cpu_vecops import CpuVecOps
from pnode_amd import _funcguard, _lib, _linearfwd, options, petsc_adjoint
from pnode_amd._lib import PnError
from problems import flat_grads, rel_err


def _shapes(dtype, rows, out_f, in_f):
    return dtype == torch.float32 and rows >= 256 and out_f % 64 == 0 and in_f % 64 == 0


class NoReluOps(CpuVecOps):
    """The CPU stand-in with the entry points of pn_linear_fwd (every activation), pn_linear_bwd and pn_linear_dx, but without the
    `linear_relu` capability: what a backend built before pn_linear_bwd_act looks like to the engine."""
    calls = {}

    @classmethod
    def count(cls, what):
        NoReluOps.calls[what] = NoReluOps.calls.get(what, 0) + 1

    def linear_fwd_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_fwd(self, x, w, b, tanh, y=None, flags=None, act=None):
        assert self.linear_fwd_supported(x.shape[0], w.shape[0], w.shape[1]) and x.dim() == 2 and x.is_contiguous()
        act = act if act is not None else ("tanh" if tanh else "identity")
        self.count("fwd_" + act)
        z = F.linear(x, w, b)
        return {"tanh": torch.tanh, "relu": torch.relu, "identity": lambda v: v}[act](z)

    def linear_bwd_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        assert g.dim() == 2 and g.is_contiguous() and a.shape == g.shape
        self.count("bwd_" + act)
        gz = torch.ops.aten.threshold_backward(g, a, 0) if act == "relu" else torch.ops.aten.tanh_backward(g, a)
        return gz, torch.matmul(gz, w)

    def linear_dx_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_dx(self, g, w, dx=None, flags=None):
        self.count("dx")
        return torch.matmul(g, w)


class ReluOps(NoReluOps):
    linear_relu = True


class WrongForwardOps(ReluOps):
    def linear_fwd(self, x, w, b, tanh, y=None, flags=None, act=None):
        return super().linear_fwd(x, w, b, tanh, act=act) + (1e-3 if act == "relu" else 0.0)


class WrongGzOps(ReluOps):
    """g_z of a ReLU pair with ONE bit wrong in one element (and dx of that g_z)."""
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        if act == "relu":
            gz = gz.clone()
            i = int(gz.reshape(-1).abs().argmax())
            gz.view(-1).view(torch.int32)[i] ^= 1
        return gz, dx


class WrongDxOps(ReluOps):
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        return gz, dx * (1.001 if act == "relu" else 1.0)


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self, ops=ReluOps):
        self._ops = ops(torch.device("cpu"), torch.float32, 256 * 64)


@pytest.fixture(autouse=True)
def _host_rules(monkeypatch):
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    NoReluOps.calls = {}
    options.clear()
    yield
    options.clear()


def _n(what):
    return NoReluOps.calls.get(what, 0)


def _fwd(f, relu="1", mode="auto", bwd_mode="auto", bare="0", ops=ReluOps):
    ode = _Ode(ops)
    fwd = _linearfwd.LinearFwd(ode)
    fwd.keep = ode                                # (LinearFwd holds its solver weakly)
    if relu is None:
        on = fwd.install(f, list(f.parameters()), mode, bwd_mode, bare)
    else:
        on = fwd.install(f, list(f.parameters()), mode, bwd_mode, bare, relu)
    return fwd, ode, on


def _y(rows=256, d=64, seed=1):
    return torch.randn(rows, d, generator=torch.Generator().manual_seed(seed))


def _seq_func(*layers):
    class Func(nn.Module):
        def __init__(self):
            super().__init__()
            self.net = nn.Sequential(*layers)

        def forward(self, t, y):
            return self.net(y)
    torch.manual_seed(7)
    return Func()


def _relu_net(d=64):
    """The func of the GPU solve test: two ReLU pairs, the second one in place, and a bare head."""
    return _seq_func(nn.Linear(d, d), nn.ReLU(), nn.Linear(d, d), nn.ReLU(inplace=True), nn.Linear(d, d))


def _eval(f, fwd, y, loss=lambda out: out.pow(2).sum()):
    with fwd.window():
        out = f(0.0, y)
    wrt = ([y] if y.requires_grad else []) + list(f.parameters())
    return out, torch.autograd.grad(loss(out), wrt)


def _stock(f, y, loss=lambda out: out.pow(2).sum()):
    out = f(0.0, y)
    return out, torch.autograd.grad(loss(out), ([y] if y.requires_grad else []) + list(f.parameters()))


def _close(gg, gw):
    return all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))


class _MyReLU(nn.ReLU):
    pass


class _MyLinear(nn.Linear):
    pass


def _plan(found):
    return [(type(s), {i: tuple(type(m) for m in p) if isinstance(p, tuple) else type(p) for i, p in d.items()}) for s, d in found]


# ------------------------------------------------------------------------------------------------------------------ finding the pairs
def test_with_1_a_linear_relu_is_a_pair_and_not_a_bare_layer():
    f = _seq_func(nn.Linear(64, 128), nn.ReLU(), nn.Linear(128, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.ReLU)})] and refused == {}
    assert plans[0][1][0] == (f.net[0], f.net[1])
    assert _plan(bare) == [(nn.Sequential, {2: nn.Linear})]
    # a tanh pair beside it is found as before; an in-place ReLU is a ReLU
    f = _seq_func(nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 64), nn.ReLU(inplace=True), nn.Linear(64, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.Tanh), 2: (nn.Linear, nn.ReLU)})] and refused == {}
    assert _plan(bare) == [(nn.Sequential, {4: nn.Linear})]
    fwd, _, on = _fwd(f, "1")
    assert on and [sorted(p) for _, p in fwd.plans] == [[0]] and [sorted(p) for _, p in fwd.relu] == [[2]]


def _funcs_for_0():
    lin = nn.Linear(64, 64)
    a, b = nn.Linear(64, 64), nn.Linear(64, 64)
    b.weight = a.weight
    return {
        "linear relu linear": (_seq_func(nn.Linear(64, 128), nn.ReLU(), nn.Linear(128, 64)), [], {}, [{0: nn.Linear, 2: nn.Linear}]),
        "relu subclass": (_seq_func(nn.Linear(64, 64), _MyReLU(), nn.Linear(64, 64)), [], {}, [{0: nn.Linear, 2: nn.Linear}]),
        "linear twice": (_seq_func(lin, nn.ReLU(), lin), [], {}, []),
        "shared weight": (_seq_func(a, nn.ReLU(), b), [], {}, []),
        "with a tanh pair": (_seq_func(nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 64), nn.ReLU()), [{0: (nn.Linear, nn.Tanh)}], {},
                             [{2: nn.Linear}]),
    }


@pytest.mark.parametrize("name", ["linear relu linear", "relu subclass", "linear twice", "shared weight", "with a tanh pair"])
def test_with_0_find_layers_gives_what_it_gave_before_there_was_the_option(name):
    f, plans_w, refused_w, bare_w = _funcs_for_0()[name]
    for args in ((), (False,)):
        plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), *args)
        assert [d for _, d in _plan(plans)] == plans_w and refused == refused_w and [d for _, d in _plan(bare)] == bare_w
    assert _linearfwd.find_pairs(f, list(f.parameters())) == tuple(_linearfwd.find_layers(f, list(f.parameters()))[:2])
    # ... and the installed solver has no ReLU pair, whatever the func
    for relu in (None, "0"):
        fwd, _, _ = _fwd(f, relu, bare="1")
        assert fwd.relu == [] and not fwd.relu_active and fwd.relu_status == "off (-pn_linear_relu 0)"
        assert [d for _, d in _plan(fwd.bare)] == bare_w and [d for _, d in _plan(fwd.plans)] == plans_w


def test_by_default_and_with_0_a_relu_net_runs_the_stock_modules_or_bare_layers_as_before():
    f = _relu_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for relu in (None, "0"):
        fwd, _, on = _fwd(f, relu)
        assert not on and not fwd.active
        got, gg = _eval(f, fwd, y)
        assert NoReluOps.calls == {} and torch.equal(got, want) and _close(gg, gw)
    fwd, _, on = _fwd(f, "0", bare="1")
    assert on and [sorted(b) for _, b in fwd.bare] == [[0, 2, 4]]
    got, gg = _eval(f, fwd, y)
    assert NoReluOps.calls == {"fwd_identity": 3, "dx": 3} and fwd.n_relu == 0 and fwd.n_relu_bwd == 0
    assert torch.equal(got, want) and _close(gg, gw)


# --------------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("what", ["relu subclass", "linear subclass", "instance forward on the relu", "instance forward on the linear",
                                  "instance forward on the container", "shared weight"])
def test_static_refusals_send_the_pair_to_the_stock_modules_and_option_fwd_1_warns_once(what):
    layers = [nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64)]
    if what == "relu subclass":
        layers[1] = _MyReLU()
    elif what == "linear subclass":
        layers[0] = _MyLinear(64, 64)
    elif what == "shared weight":
        layers[2].weight = layers[0].weight
    f = _seq_func(*layers)
    if what == "instance forward on the relu":
        f.net[1].forward = lambda x: torch.relu(x)
    elif what == "instance forward on the linear":
        f.net[0].forward = lambda x: F.linear(x, f.net[0].weight, f.net[0].bias)
    elif what == "instance forward on the container":
        f.net.forward = lambda x: f.net[2](f.net[1](f.net[0](x)))
    before = _funcguard.snapshot([f])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fwd, _, on = _fwd(f, "1", mode="1")
        y = _y()
        with fwd.window():
            got = f(0.0, y)
        with fwd.window():
            f(0.0, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_fwd 1: a Linear -> ReLU pair" in str(c.message)]
    assert len(msgs) == 1 and "runs the stock modules" in msgs[0], [str(c.message) for c in caught]
    assert not on and fwd.relu == [] and NoReluOps.calls == {} and fwd.n_relu == 0
    assert fwd.relu_status == "stock modules (no eligible Linear -> ReLU pair)"
    assert torch.equal(got, f(0.0, y)) and _funcguard.snapshot([f]) == before


@pytest.mark.parametrize("where", ["linear", "relu", "container", "pre", "backward"])
def test_a_user_hook_on_the_pair_or_its_container_runs_the_stock_modules(where):
    f = _relu_net()
    fwd, _, on = _fwd(f, "1", mode="1")
    assert on and [sorted(p) for _, p in fwd.relu] == [[0, 2]]
    before = _funcguard.snapshot([f])
    seen = []
    if where == "pre":
        h = f.net[0].register_forward_pre_hook(lambda m, i: seen.append("pre"))
    elif where == "backward":
        h = f.net[1].register_full_backward_hook(lambda m, gi, go: None)
    else:
        m = {"linear": f.net[0], "relu": f.net[3], "container": f.net}[where]
        h = m.register_forward_hook(lambda m, i, o: seen.append(where))
    y = _y()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):
            with fwd.window():
                assert "forward" not in f.net.__dict__
                got = f(0.0, y)
    msgs = [str(c.message) for c in caught if "a Linear -> ReLU pair runs the stock modules" in str(c.message)]
    assert len(msgs) == 1 and "hook on the pair or its container" in msgs[0]
    assert NoReluOps.calls == {} and torch.equal(got, f(0.0, y))
    if where != "backward":
        assert seen
    h.remove()
    assert _funcguard.snapshot([f]) == before
    with fwd.window():
        f(0.0, y)
    assert NoReluOps.calls == {"fwd_relu": 2} and fwd.n_relu == 2


def test_call_time_refusals_run_the_stock_modules():
    f = _relu_net()
    fwd, _, _ = _fwd(f, "1")
    y = _y()
    before = _funcguard.snapshot([f])
    with fwd.window():
        with torch.autocast("cpu", dtype=torch.bfloat16):
            f(0.0, y)
        assert NoReluOps.calls == {}
        got = f(0.0, _y(rows=128))                # outside pn_linear_fwd_supported
        assert NoReluOps.calls == {} and torch.equal(got, f.net(_y(rows=128)))
        f(0.0, y)
    assert NoReluOps.calls == {"fwd_relu": 2} and _funcguard.snapshot([f]) == before and "forward" not in f.net.__dict__


def test_func_is_left_as_found_also_when_an_evaluation_raises():
    class Boom(nn.Module):
        def forward(self, x):
            raise ValueError("boom")
    f = _seq_func(nn.Linear(64, 64), nn.ReLU(), Boom())
    fwd, _, on = _fwd(f, "1")
    assert on
    before = _funcguard.snapshot([f])
    with fwd.window():
        assert "forward" in f.net.__dict__
    assert _funcguard.snapshot([f]) == before and "forward" not in f.net.__dict__
    with pytest.raises(ValueError, match="boom"):
        with fwd.window():
            f(0.0, _y())
    assert _n("fwd_relu") == 1
    assert _funcguard.snapshot([f]) == before and "forward" not in f.net.__dict__


# ------------------------------------------------------------------------------------------------------------------- running the pairs
@pytest.mark.parametrize("bare", ["0", "1"])
def test_output_and_gradients_are_the_stock_modules_and_the_counters_are_the_relu_pairs_own(bare):
    f = _relu_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, "1", bare=bare)
    assert on and fwd.active and fwd.plans == [] and [sorted(p) for _, p in fwd.relu] == [[0, 2]]
    assert [sorted(b) for _, b in fwd.bare] == [[4]]
    got, gg = _eval(f, fwd, y)
    assert torch.equal(got, want) and _close(gg, gw)
    assert torch.equal(gg[0], gw[0])              # dL/dy: threshold_backward and matmul on both sides
    assert fwd.n_relu == 2 and fwd.n_relu_bwd == 2 and fwd.n_fused == 0 and fwd.n_fused_bwd == 0
    assert _n("fwd_relu") == 2 and _n("bwd_relu") == 2 and _n("fwd_tanh") == 0 and _n("bwd_tanh") == 0
    assert (fwd.n_bare, _n("fwd_identity"), _n("dx")) == ((1, 1, 1) if bare == "1" else (0, 0, 0))
    assert fwd.relu_checked and fwd.relu_bwd_checked and not fwd.relu_disabled and not fwd.relu_bwd_disabled
    assert fwd.relu_status == "fused (2 pairs; 2 forward, 2 backward calls so far)"
    assert "forward" not in f.net.__dict__
    f(0.0, y)                                     # outside the window: the stock modules
    assert _n("fwd_relu") == 2
    # the in-place ReLU was not called: the fused output is nobody's input buffer
    assert f.net[3].inplace and torch.equal(_eval(f, fwd, y)[0], want)


def test_an_input_that_needs_no_gradient_and_a_cotangent_that_is_not_contiguous():
    f = _relu_net()
    fwd, _, _ = _fwd(f, "1")
    _, gg = _eval(f, fwd, _y())
    assert fwd.n_relu == 2 and fwd.n_relu_bwd == 1 and _close(gg, _stock(f, _y())[1])      # the first pair forms no dx at all
    assert _n("bwd_relu") == 1
    NoReluOps.calls = {}
    one = _seq_func(nn.Linear(64, 64), nn.ReLU())
    fwd, _, _ = _fwd(one, "1")
    y = _y().requires_grad_(True)
    _, gg = _eval(one, fwd, y, lambda out: out.sum())                                      # expanded by sum: not contiguous
    assert fwd.n_relu == 1 and fwd.n_relu_bwd == 0 and _n("bwd_relu") == 0 and _close(gg, _stock(one, y, lambda out: out.sum())[1])


def test_a_relu_forward_off_by_a_thousandth_switches_off_the_relu_pairs_only():
    f = _seq_func(nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64))
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, ode, _ = _fwd(f, "1", ops=WrongForwardOps)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        got2, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> ReLU forward is switched off" in str(c.message)]
    assert len(msgs) == 1 and "torch.relu(F.linear) differ by" in msgs[0]
    assert fwd.relu_disabled and fwd.n_relu == 0 and _n("fwd_relu") == 1 and not fwd.relu_active
    assert fwd.relu_status.startswith("stock modules (pn_linear_fwd and torch.relu(F.linear) differ by")
    # the tanh pair of the same func stays fused, forward and backward
    assert not fwd.disabled and fwd.n_fused == 2 and not fwd.bwd_disabled and fwd.n_fused_bwd == 2 and fwd.active
    assert torch.equal(got, want) and torch.equal(got2, want) and _close(g1, gw) and _close(g2, gw)


@pytest.mark.parametrize("ops,what", [(WrongGzOps, "g_z is not threshold_backward's bit for bit"), (WrongDxOps, "dx by")])
def test_a_wrong_relu_backward_switches_off_the_relu_backward_only(ops, what):
    f = _seq_func(nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64))
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, "1", ops=ops)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        _, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> ReLU backward is switched off" in str(c.message)]
    assert len(msgs) == 1 and what in msgs[0]
    assert fwd.relu_bwd_disabled and fwd.n_relu_bwd == 0 and _n("bwd_relu") == 1 and what in fwd.relu_bwd_why
    assert "pn_linear_bwd_act and threshold_backward + matmul differ" in fwd.relu_bwd_why
    # the ReLU forward and the tanh pair, forward and backward, stay fused
    assert not fwd.relu_disabled and fwd.n_relu == 2 and fwd.relu_status == "fused (1 pairs; 2 forward, 0 backward calls so far)"
    assert not fwd.disabled and fwd.n_fused == 2 and not fwd.bwd_disabled and fwd.n_fused_bwd == 2
    assert torch.equal(got, want) and _close(g1, gw) and _close(g2, gw)


def test_option_bwd_0_and_a_backend_without_linear_relu_run_threshold_backward_and_matmul():
    f = _relu_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for kw in ({"bwd_mode": "0"}, {"ops": NoReluOps}):
        NoReluOps.calls = {}
        fwd, _, _ = _fwd(f, "1", **kw)
        got, gg = _eval(f, fwd, y)
        assert fwd.n_relu == 2 and _n("fwd_relu") == 2 and fwd.n_relu_bwd == 0 and _n("bwd_relu") == 0
        assert torch.equal(got, want) and torch.equal(gg[0], gw[0]) and _close(gg, gw)
    # -pn_linear_bwd 1 says why, once, in the wording of a tanh pair
    fwd, _, _ = _fwd(f, "1", bwd_mode="1", ops=NoReluOps)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_bwd 1" in str(c.message)]
    assert msgs == ["pnode_amd: -pn_linear_bwd 1: the backward of a Linear -> ReLU pair runs the torch operations: the backend has no linear_relu"]


# --------------------------------------------------------------------------------------------------------------- solves and the option
def _solve(f, relu, backend=ReluOps, steps=3, **more):
    options.clear()
    options.set_option("ts_adapt_type", "none")
    if relu is not None:
        options.set_option("pn_linear_relu", relu)
    for k, v in more.items():
        options.set_option(k, v)
    y0 = _y()
    ode = petsc_adjoint.ODEPetsc(backend=backend)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    for p in f.parameters():
        p.grad = None
    y = y0.clone().requires_grad_(True)
    out = ode.odeint_adjoint(y, torch.tensor([0.0, 0.05 * steps], dtype=torch.float64))
    out[-1].pow(2).sum().backward()
    return out.detach().clone(), y.grad.clone(), flat_grads(f).clone(), ode


def test_a_whole_solve_and_the_three_statuses():
    f = _relu_net()
    o0, y0, p0, ode0 = _solve(f, None)
    assert ode0._fwd is None and ode0.linear_relu == "off (-pn_linear_relu 0)" and NoReluOps.calls == {}
    oz, yz, pz, odez = _solve(f, "0", pn_linear_bare=1)
    assert odez.linear_relu == "off (-pn_linear_relu 0)" and odez._fwd.n_relu == 0 and odez._fwd.n_bare > 0 and _n("fwd_relu") == 0
    o1, y1, p1, ode1 = _solve(f, "1", pn_linear_bare=1)
    fwd = ode1._fwd
    # rk4 x 3 steps: at least four stage evaluations and four stage VJPs per step, two ReLU pairs each
    assert fwd.n_relu >= 3 * 4 * 2 * 2 and fwd.n_relu_bwd >= 3 * 4 * 2 and fwd.n_fused == 0 and fwd.n_fused_bwd == 0
    assert 2 * fwd.n_bare == fwd.n_relu and 2 * fwd.n_bare_bwd == fwd.n_relu_bwd
    assert ode1.linear_relu == "fused (2 pairs; %d forward, %d backward calls so far)" % (fwd.n_relu, fwd.n_relu_bwd)
    assert ode1.linear_bare.startswith("fused (1 layers") and ode1.linear_fwd.startswith("stock modules")
    assert ode1.linear_param_grads.startswith("engine") and ode1._lin.n_autograd == 0 and ode1._lin.n_clean > 0
    for o, y, p in ((oz, yz, pz), (o1, y1, p1)):
        assert torch.equal(o, o0) and rel_err(y, y0) < 1e-6 and rel_err(p, p0) < 1e-6
    # nothing to fuse: the third string
    g = _seq_func(nn.Linear(64, 64), _MyReLU(), nn.Linear(64, 64))
    _, _, _, ode = _solve(g, "1", pn_linear_bare=1)
    assert ode.linear_relu == "stock modules (no eligible Linear -> ReLU pair)"
    _, _, _, ode = _solve(g, "1")
    assert ode._fwd is None and ode.linear_relu.startswith("stock modules (no eligible pair")
    # -pn_linear_fwd 0 switches the ReLU pairs off with the tanh pairs; an fp64 state has none
    _, _, _, ode = _solve(f, "1", pn_linear_fwd=0)
    assert ode._fwd is None and ode.linear_relu.startswith("stock modules") and _n("fwd_relu") == fwd.n_relu


def test_any_other_value_of_the_option_is_refused():
    f = _relu_net()
    for bad in ("2", "auto", "-1", "yes"):
        with pytest.raises(PnError, match="-pn_linear_relu must be 0 or 1"):
            _solve(f, bad)


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def _last_error(lib):
    return lib.pn_last_error().decode()


def test_pn_linear_bwd_act_refuses_by_name_and_launches_nothing():
    lib = _lib.load()
    assert (_lib.PN_ACT_IDENTITY, _lib.PN_ACT_TANH, _lib.PN_ACT_RELU) == (0, 1, 2)
    n = 256 * 64
    big = torch.zeros(5 * n + 8)
    g, a, w, gz, dx = (big.data_ptr() + 4 * n * k for k in range(5))
    assert g % 16 == 0
    RELU, PLAIN = _lib.PN_ACT_RELU, _lib.PN_LINEAR_FORM_PLAIN

    def call(pg, pa, pw, pgz, pdx, act=RELU, flags=0, rows=256, dtype=0):
        return lib.pn_linear_bwd_act(None, dtype, rows, 64, 64, pg, pa, pw, act, pgz, pdx, flags)
    ok = (g, a, w, gz, dx)
    # an unknown flag first, whatever else holds
    for flags in (2, 4, 3, -2):
        assert call(*ok, flags=flags) != 0 and "pn_linear_bwd_act: unknown flag" in _last_error(lib) and "PN_LINEAR_FORM_PLAIN" in _last_error(lib)
        assert call(*ok, flags=flags, act=7, rows=128) != 0 and "pn_linear_bwd_act: unknown flag" in _last_error(lib)
    for flags in (0, PLAIN):
        assert call(*ok, act=_lib.PN_ACT_IDENTITY, flags=flags) != 0 and "use pn_linear_dx" in _last_error(lib)
        for act in (7, 3, -1):
            assert call(*ok, act=act, flags=flags) != 0
            assert "act is PN_ACT_TANH or PN_ACT_RELU" in _last_error(lib) and "pn_linear_dx" in _last_error(lib)
        for act in (_lib.PN_ACT_TANH, RELU):
            assert call(*ok, act=act, flags=flags, rows=128) != 0 and "pn_linear_bwd: unsupported dtype or shape" in _last_error(lib)
            assert call(*ok, act=act, flags=flags, dtype=1) != 0 and "pn_linear_bwd: unsupported dtype or shape" in _last_error(lib)
            for k in range(5):
                assert call(*[None if j == k else p for j, p in enumerate(ok)], act=act, flags=flags) != 0 and "null operand" in _last_error(lib)
                assert call(*[p + 4 if j == k else p for j, p in enumerate(ok)], act=act, flags=flags) != 0 and "16-byte aligned" in _last_error(lib)
            for alias in (g, a, w, g + 16):
                assert call(g, a, w, alias, dx, act=act, flags=flags) != 0 and "gz must not alias g, a or w" in _last_error(lib)
            for alias in (g, a, w, gz, gz + 4 * n - 16):
                assert call(g, a, w, gz, alias, act=act, flags=flags) != 0 and "dx must not alias g, a, w or gz" in _last_error(lib)
    assert not bool(big.any())
    # pn_linear_fwd names the three activations it takes
    p = big.data_ptr()
    assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, 7, p) != 0
    assert "pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU" in _last_error(lib)
    assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, RELU, p) != 0 and "y must not alias" in _last_error(lib)
