"""func's nn.Linear -> nn.Sigmoid pairs (pnode_amd/_linearfwd.py, ``-pn_linear_sigmoid 0|1``): which children are such a pair, that the
default changes nothing, what every other case falls back to, the self-checks of their own with their absolute term, and the C entry
point's refusals.  Host logic: ``pn_linear_fwd`` with ``PN_ACT_SIGMOID`` and ``pn_linear_bwd_act`` are stood in for by the torch
expressions they replace (``sigmoid(F.linear)``; ``sigmoid_backward`` and ``matmul``), so every output must EQUAL the stock modules' and
every gradient agrees with autograd's to 1e-6 in the relative 2-norm (one sum formed by ``mm`` here and by ``addmm`` /
``linear_backward`` there: the bar of tests/test_linear_bare.py)."""
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _cpu_vecops import CpuVecOps
from pnode_amd import _funcguard, _lib, _linearfwd, options, petsc_adjoint
from pnode_amd._lib import PnError
from problems import DiffusionIM, flat_grads, rel_err

_ACT = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, "identity": lambda v: v}


def _shapes(dtype, rows, out_f, in_f):
    return dtype == torch.float32 and rows >= 256 and out_f % 64 == 0 and in_f % 64 == 0


class NoSigmoidOps(CpuVecOps):
    """The CPU stand-in with the entry points of pn_linear_fwd (every activation), pn_linear_bwd and pn_linear_dx and the ReLU
    capability, but without `linear_sigmoid`: what a backend built before PN_ACT_SIGMOID looks like to the engine."""
    linear_relu = True
    calls = {}

    @classmethod
    def count(cls, what):
        NoSigmoidOps.calls[what] = NoSigmoidOps.calls.get(what, 0) + 1

    def linear_fwd_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_fwd(self, x, w, b, tanh, y=None, flags=None, act=None):
        assert self.linear_fwd_supported(x.shape[0], w.shape[0], w.shape[1]) and x.dim() == 2 and x.is_contiguous()
        act = act if act is not None else ("tanh" if tanh else "identity")
        self.count("fwd_" + act)
        return _ACT[act](F.linear(x, w, b))

    def linear_bwd_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        assert g.dim() == 2 and g.is_contiguous() and a.shape == g.shape
        self.count("bwd_" + act)
        if act == "sigmoid":
            gz = torch.ops.aten.sigmoid_backward(g, a)
        else:
            gz = torch.ops.aten.threshold_backward(g, a, 0) if act == "relu" else torch.ops.aten.tanh_backward(g, a)
        return gz, torch.matmul(gz, w)

    def linear_dx_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_dx(self, g, w, dx=None, flags=None):
        self.count("dx")
        return torch.matmul(g, w)


class SigmoidOps(NoSigmoidOps):
    linear_sigmoid = True


class WrongForwardOps(SigmoidOps):
    def linear_fwd(self, x, w, b, tanh, y=None, flags=None, act=None):
        return super().linear_fwd(x, w, b, tanh, act=act) + (1e-3 if act == "sigmoid" else 0.0)


class TwoUlpOnZeroRowsOps(SigmoidOps):
    """A Sigmoid forward that is off by 2 ulp (of 0.5: 2 * 2^-24) on the rows whose x is zero -- with a zero bias their pre-activation is
    an exact 0 and sum |x w| + |b| is 0: only the absolute term of the bar covers them."""
    def linear_fwd(self, x, w, b, tanh, y=None, flags=None, act=None):
        out = super().linear_fwd(x, w, b, tanh, act=act)
        if act == "sigmoid":
            zero = (x == 0).all(1)
            assert bool(zero.any()) and bool((out[zero] == 0.5).all())
            out = out.clone()
            out[zero] += 2.0 * 2.0 ** -24
        return out


def _bar(g):
    return 1.5 * 2.0 ** -24 * g.abs()              # (the engine's expression, in fp32 as there)


class WrongGzOps(SigmoidOps):
    """g_z of a Sigmoid pair with one element ONE bit beyond the bar 1.5 * 2^-24 |g| (and dx of the right g_z)."""
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        if act == "sigmoid":
            gz = gz.clone()
            i = int(g.reshape(-1).abs().argmax())
            right, bar = gz.view(-1)[i].clone(), _bar(g.reshape(-1)[i])
            v = right + bar
            while bool((v - right).abs() <= bar):
                v = torch.nextafter(v, torch.tensor(float("inf")))
            assert bool((torch.nextafter(v, torch.tensor(-float("inf"))) - right).abs() <= bar)
            gz.view(-1)[i] = v
        return gz, dx


class GzAtTheBarOps(SigmoidOps):
    """... and with EVERY element moved as far as the bar lets it: no miss."""
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        if act == "sigmoid":
            v = gz + _bar(g)
            v = torch.where((v - gz).abs() <= _bar(g), v, torch.nextafter(v, torch.full_like(v, -float("inf"))))
            assert bool(((v - gz).abs() <= _bar(g)).all()) and not torch.equal(v, gz)
            gz = v
        return gz, dx


class WrongDxOps(SigmoidOps):
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        return gz, dx * (1.001 if act == "sigmoid" else 1.0)


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self, ops=SigmoidOps):
        self._ops = ops(torch.device("cpu"), torch.float32, 256 * 64)


@pytest.fixture(autouse=True)
def _host_rules(monkeypatch):
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    NoSigmoidOps.calls = {}
    options.clear()
    yield
    options.clear()


def _n(what):
    return NoSigmoidOps.calls.get(what, 0)


def _fwd(f, sigmoid="1", mode="auto", bwd_mode="auto", bare="0", relu="0", ops=SigmoidOps):
    ode = _Ode(ops)
    fwd = _linearfwd.LinearFwd(ode)
    fwd.keep = ode                                # (LinearFwd holds its solver weakly)
    if sigmoid is None:
        on = fwd.install(f, list(f.parameters()), mode, bwd_mode, bare, relu)
    else:
        on = fwd.install(f, list(f.parameters()), mode, bwd_mode, bare, relu, sigmoid_mode=sigmoid)
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


def _sigmoid_net(d=64):
    """The func of the GPU solve test: two Sigmoid pairs and a bare head (the shape of the KS workload's ODEFunc)."""
    return _seq_func(nn.Linear(d, d), nn.Sigmoid(), nn.Linear(d, d), nn.Sigmoid(), nn.Linear(d, d))


def _mixed_net(d=64):
    return _seq_func(nn.Linear(d, d), nn.ReLU(), nn.Linear(d, d), nn.Sigmoid(), nn.Linear(d, d), nn.Tanh(), nn.Linear(d, d))


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


class _MySigmoid(nn.Sigmoid):
    pass


def _plan(found):
    return [(type(s), {i: tuple(type(m) for m in p) if isinstance(p, tuple) else type(p) for i, p in d.items()}) for s, d in found]


# ------------------------------------------------------------------------------------------------------------------ finding the pairs
def test_with_sigmoid_a_linear_sigmoid_is_a_pair_and_not_a_bare_layer():
    f = _seq_func(nn.Linear(64, 128), nn.Sigmoid(), nn.Linear(128, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), sigmoid=True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.Sigmoid)})] and refused == {}
    assert plans[0][1][0] == (f.net[0], f.net[1])
    assert _plan(bare) == [(nn.Sequential, {2: nn.Linear})]
    # the other kinds beside it are found as before, each under its own keyword
    f = _mixed_net()
    params = list(f.parameters())
    plans, refused, bare = _linearfwd.find_layers(f, params, True, sigmoid=True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.ReLU), 2: (nn.Linear, nn.Sigmoid), 4: (nn.Linear, nn.Tanh)})] and refused == {}
    assert _plan(bare) == [(nn.Sequential, {6: nn.Linear})]
    plans, _, bare = _linearfwd.find_layers(f, params, sigmoid=True)
    assert _plan(plans) == [(nn.Sequential, {2: (nn.Linear, nn.Sigmoid), 4: (nn.Linear, nn.Tanh)})]
    assert _plan(bare) == [(nn.Sequential, {0: nn.Linear, 6: nn.Linear})]
    fwd, _, on = _fwd(f, "1", relu="1")
    assert on and [sorted(p) for _, p in fwd.plans] == [[4]] and [sorted(p) for _, p in fwd.relu] == [[0]]
    assert [sorted(p) for _, p in fwd.sigmoid] == [[2]] and fwd.sigmoid_active


def test_a_subclass_of_sigmoid_is_no_pair():
    f = _seq_func(nn.Linear(64, 64), _MySigmoid(), nn.Linear(64, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), sigmoid=True)
    assert plans == [] and refused == {("Sequential", "Sigmoid"): "a subclass of nn.Linear or nn.Sigmoid"}
    assert _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear})]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fwd, _, on = _fwd(f, "1", mode="1")
        y = _y()
        for _ in range(2):
            with fwd.window():
                got = f(0.0, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_fwd 1: a Linear -> Sigmoid pair" in str(c.message)]
    assert len(msgs) == 1 and "runs the stock modules" in msgs[0], [str(c.message) for c in caught]
    assert not on and fwd.sigmoid == [] and NoSigmoidOps.calls == {} and fwd.n_sigmoid == 0
    assert fwd.sigmoid_status == "stock modules (no eligible Linear -> Sigmoid pair)"
    assert torch.equal(got, f(0.0, y))


@pytest.mark.parametrize("where", ["linear", "sigmoid", "container", "pre", "backward"])
def test_a_user_hook_on_the_pair_or_its_container_runs_the_stock_modules(where):
    f = _sigmoid_net()
    fwd, _, on = _fwd(f, "1", mode="1")
    assert on and [sorted(p) for _, p in fwd.sigmoid] == [[0, 2]]
    before = _funcguard.snapshot([f])
    seen = []
    if where == "pre":
        h = f.net[0].register_forward_pre_hook(lambda m, i: seen.append("pre"))
    elif where == "backward":
        h = f.net[1].register_full_backward_hook(lambda m, gi, go: None)
    else:
        m = {"linear": f.net[0], "sigmoid": f.net[3], "container": f.net}[where]
        h = m.register_forward_hook(lambda m, i, o: seen.append(where))
    y = _y()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):
            with fwd.window():
                assert "forward" not in f.net.__dict__
                got = f(0.0, y)
    msgs = [str(c.message) for c in caught if "a Linear -> Sigmoid pair runs the stock modules" in str(c.message)]
    assert len(msgs) == 1 and "hook on the pair or its container" in msgs[0]
    assert NoSigmoidOps.calls == {} and torch.equal(got, f(0.0, y))
    if where != "backward":
        assert seen
    h.remove()
    assert _funcguard.snapshot([f]) == before
    with fwd.window():
        f(0.0, y)
    assert NoSigmoidOps.calls == {"fwd_sigmoid": 2} and fwd.n_sigmoid == 2


def test_with_0_or_absent_plans_bare_layers_and_outputs_are_what_they_are_today():
    f = _sigmoid_net()
    params = list(f.parameters())
    for args, kw in (((), {}), ((False,), {}), ((True,), {}), ((), {"sigmoid": False})):
        plans, refused, bare = _linearfwd.find_layers(f, params, *args, **kw)
        assert plans == [] and refused == {} and _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear, 4: nn.Linear})]
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for sigmoid in (None, "0"):
        fwd, _, on = _fwd(f, sigmoid)
        assert not on and not fwd.active and fwd.sigmoid == [] and fwd.sigmoid_status == "off (-pn_linear_sigmoid 0)"
        got, gg = _eval(f, fwd, y)
        assert NoSigmoidOps.calls == {} and torch.equal(got, want) and _close(gg, gw)
    # under -pn_linear_bare 1 a Linear in front of a Sigmoid is a bare layer
    for sigmoid in (None, "0"):
        NoSigmoidOps.calls = {}
        fwd, _, on = _fwd(f, sigmoid, bare="1")
        assert on and [sorted(b) for _, b in fwd.bare] == [[0, 2, 4]] and fwd.sigmoid == [] and not fwd.sigmoid_active
        got, gg = _eval(f, fwd, y)
        assert NoSigmoidOps.calls == {"fwd_identity": 3, "dx": 3} and fwd.n_sigmoid == 0 and fwd.n_sigmoid_bwd == 0
        assert torch.equal(got, want) and _close(gg, gw)


def test_a_call_time_refusal_runs_the_stock_modules_and_its_reason_is_in_the_status():
    f = _sigmoid_net()
    fwd, _, _ = _fwd(f, "1")
    before = _funcguard.snapshot([f])
    with fwd.window():
        got = f(0.0, _y(rows=128))                # outside pn_linear_fwd_supported
    assert NoSigmoidOps.calls == {} and torch.equal(got, f.net(_y(rows=128))) and _funcguard.snapshot([f]) == before
    assert fwd.sigmoid_status == ("fused (2 pairs; 0 forward, 0 backward calls so far; the stock modules where a call is refused, last: "
                                  "outside pn_linear_fwd_supported)")
    with fwd.window():
        f(0.0, _y())
    assert NoSigmoidOps.calls == {"fwd_sigmoid": 2} and fwd.sigmoid_status.startswith("fused (2 pairs; 2 forward, 0 backward calls so far;")


# ------------------------------------------------------------------------------------------------------------------- running the pairs
@pytest.mark.parametrize("bare", ["0", "1"])
def test_output_and_gradients_are_the_stock_modules_and_the_counters_are_the_sigmoid_pairs_own(bare):
    f = _sigmoid_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, "1", bare=bare)
    assert on and fwd.active and fwd.plans == [] and fwd.relu == [] and [sorted(p) for _, p in fwd.sigmoid] == [[0, 2]]
    assert [sorted(b) for _, b in fwd.bare] == [[4]]
    got, gg = _eval(f, fwd, y)
    assert torch.equal(got, want) and _close(gg, gw)
    assert torch.equal(gg[0], gw[0])              # dL/dy: sigmoid_backward and matmul on both sides
    assert fwd.n_sigmoid == 2 and fwd.n_sigmoid_bwd == 2 and fwd.n_fused == 0 and fwd.n_fused_bwd == 0 and fwd.n_relu == 0 and fwd.n_relu_bwd == 0
    assert _n("fwd_sigmoid") == 2 and _n("bwd_sigmoid") == 2 and _n("fwd_tanh") == 0 and _n("bwd_tanh") == 0 and _n("fwd_relu") == 0
    assert (fwd.n_bare, _n("fwd_identity"), _n("dx")) == ((1, 1, 1) if bare == "1" else (0, 0, 0))
    assert fwd.sig.checked and fwd.sig.bwd_checked and not fwd.sig.disabled and not fwd.sig.bwd_disabled
    assert fwd.sigmoid_status == "fused (2 pairs; 2 forward, 2 backward calls so far)"
    assert "forward" not in f.net.__dict__
    f(0.0, y)                                     # outside the window: the stock modules
    assert _n("fwd_sigmoid") == 2


def test_a_mixed_net_counts_each_kind_once_per_evaluation_and_the_head_is_bare():
    f = _mixed_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, "1", bare="1", relu="1")
    assert on and [sorted(b) for _, b in fwd.bare] == [[6]]
    for k in (1, 2):
        got, gg = _eval(f, fwd, y)
        assert torch.equal(got, want) and _close(gg, gw)
        assert (fwd.n_fused, fwd.n_relu, fwd.n_sigmoid, fwd.n_bare) == (k, k, k, k)
        assert (fwd.n_fused_bwd, fwd.n_relu_bwd, fwd.n_sigmoid_bwd, fwd.n_bare_bwd) == (k, k, k, k)
        assert NoSigmoidOps.calls == {"fwd_relu": k, "fwd_sigmoid": k, "fwd_tanh": k, "fwd_identity": k,
                                      "bwd_relu": k, "bwd_sigmoid": k, "bwd_tanh": k, "dx": k}
    assert fwd.sigmoid_status == "fused (1 pairs; 2 forward, 2 backward calls so far)"
    assert fwd.relu_status == "fused (1 pairs; 2 forward, 2 backward calls so far)"


def test_option_bwd_0_and_a_backend_without_linear_sigmoid_run_sigmoid_backward_and_matmul():
    f = _sigmoid_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for kw in ({"bwd_mode": "0"}, {"ops": NoSigmoidOps}):
        NoSigmoidOps.calls = {}
        fwd, _, _ = _fwd(f, "1", **kw)
        got, gg = _eval(f, fwd, y)
        assert fwd.n_sigmoid == 2 and _n("fwd_sigmoid") == 2 and fwd.n_sigmoid_bwd == 0 and _n("bwd_sigmoid") == 0
        assert torch.equal(got, want) and torch.equal(gg[0], gw[0]) and _close(gg, gw)
    # -pn_linear_bwd 1 says why, once, in the wording of a tanh pair
    fwd, _, _ = _fwd(f, "1", bwd_mode="1", ops=NoSigmoidOps)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_bwd 1" in str(c.message)]
    assert msgs == ["pnode_amd: -pn_linear_bwd 1: the backward of a Linear -> Sigmoid pair runs the torch operations: "
                    "the backend has no linear_sigmoid"]


# ---------------------------------------------------------------------------------------------------------------------- the self-checks
def _others_untouched(fwd, k=2):
    """The tanh and ReLU pairs of the mixed net stay fused, forward and backward."""
    assert not fwd.disabled and not fwd.bwd_disabled and fwd.n_fused == k and fwd.n_fused_bwd == k
    assert not fwd.relu_disabled and not fwd.relu_bwd_disabled and fwd.n_relu == k and fwd.n_relu_bwd == k and fwd.active


def test_a_sigmoid_forward_off_by_a_thousandth_switches_off_the_sigmoid_pairs_only():
    f = _mixed_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, ode, _ = _fwd(f, "1", relu="1", ops=WrongForwardOps)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        got2, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> Sigmoid forward is switched off" in str(c.message)]
    assert len(msgs) == 1 and "torch.sigmoid(F.linear) differ by" in msgs[0]
    assert fwd.sig.disabled and fwd.n_sigmoid == 0 and _n("fwd_sigmoid") == 1 and not fwd.sigmoid_active
    assert fwd.sigmoid_status.startswith("stock modules (pn_linear_fwd and torch.sigmoid(F.linear) differ by")
    _others_untouched(fwd)
    assert torch.equal(got, want) and torch.equal(got2, want) and _close(g1, gw) and _close(g2, gw)


@pytest.mark.parametrize("ops,what", [(WrongGzOps, "g_z by more than 1.5 * 2^-24 |g|"), (WrongDxOps, "dx by")])
def test_a_wrong_sigmoid_backward_switches_off_the_sigmoid_backward_only(ops, what):
    f = _mixed_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, "1", relu="1", ops=ops)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        _, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> Sigmoid backward is switched off" in str(c.message)]
    assert len(msgs) == 1 and what in msgs[0]
    assert fwd.sig.bwd_disabled and fwd.n_sigmoid_bwd == 0 and _n("bwd_sigmoid") == 1 and what in fwd.sig.bwd_why
    assert "pn_linear_bwd_act and sigmoid_backward + matmul differ" in fwd.sig.bwd_why
    # the Sigmoid forward stays fused
    assert not fwd.sig.disabled and fwd.n_sigmoid == 2 and fwd.sigmoid_status == "fused (1 pairs; 2 forward, 0 backward calls so far)"
    _others_untouched(fwd)
    assert torch.equal(got, want) and _close(g1, gw) and _close(g2, gw)


def test_a_g_z_moved_as_far_as_the_bar_lets_it_is_no_miss():
    f = _sigmoid_net()
    y = _y().requires_grad_(True)
    fwd, _, _ = _fwd(f, "1", ops=GzAtTheBarOps)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _eval(f, fwd, y)
    assert fwd.sig.bwd_checked and not fwd.sig.bwd_disabled and fwd.n_sigmoid_bwd == 2


def test_two_ulp_at_a_zero_pre_activation_do_not_trip_the_forward_check():
    f = _seq_func(nn.Linear(64, 64), nn.Sigmoid(), nn.Linear(64, 64))
    with torch.no_grad():
        f.net[0].bias.zero_()
    y = _y()
    y[::3] = 0.0                                  # rows of scale 0: x = 0 and b = 0
    fwd, _, _ = _fwd(f, "1", ops=TwoUlpOnZeroRowsOps)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with fwd.window():
            got = f(0.0, y)
    assert fwd.sig.checked and not fwd.sig.disabled and fwd.n_sigmoid == 1 and fwd.sigmoid_status.startswith("fused (1 pairs; 1 forward")
    assert not torch.equal(got, f(0.0, y)) and rel_err(got, f(0.0, y)) < 1e-6
    # ... and without a bias at all
    g = _seq_func(nn.Linear(64, 64, bias=False), nn.Sigmoid())
    fwd, _, _ = _fwd(g, "1", ops=TwoUlpOnZeroRowsOps)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with fwd.window():
            g(0.0, y)
    assert not fwd.sig.disabled and fwd.n_sigmoid == 1


# --------------------------------------------------------------------------------------------------------------- solves and the option
def _solve(f, sigmoid, backend=SigmoidOps, steps=3, **more):
    options.clear()
    options.set_option("ts_adapt_type", "none")
    if sigmoid is not None:
        options.set_option("pn_linear_sigmoid", sigmoid)
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
    f = _sigmoid_net()
    o0, y0, p0, ode0 = _solve(f, None)
    assert ode0._fwd is None and ode0.linear_sigmoid == "off (-pn_linear_sigmoid 0)" and NoSigmoidOps.calls == {}
    oz, yz, pz, odez = _solve(f, "0", pn_linear_bare=1)
    assert odez.linear_sigmoid == "off (-pn_linear_sigmoid 0)" and odez._fwd.n_sigmoid == 0 and odez._fwd.n_bare > 0 and _n("fwd_sigmoid") == 0
    o1, y1, p1, ode1 = _solve(f, "1", pn_linear_bare=1)
    fwd = ode1._fwd
    # rk4 x 3 steps: at least four stage evaluations and four stage VJPs per step, two Sigmoid pairs each
    assert fwd.n_sigmoid >= 3 * 4 * 2 * 2 and fwd.n_sigmoid_bwd >= 3 * 4 * 2 and fwd.n_fused == 0 and fwd.n_relu == 0
    assert 2 * fwd.n_bare == fwd.n_sigmoid and 2 * fwd.n_bare_bwd == fwd.n_sigmoid_bwd
    assert ode1.linear_sigmoid == "fused (2 pairs; %d forward, %d backward calls so far)" % (fwd.n_sigmoid, fwd.n_sigmoid_bwd)
    assert ode1.linear_bare.startswith("fused (1 layers") and ode1.linear_fwd.startswith("stock modules")
    assert ode1.linear_relu == "off (-pn_linear_relu 0)"
    assert ode1.linear_param_grads.startswith("engine") and ode1._lin.n_autograd == 0 and ode1._lin.n_clean > 0
    for o, y, p in ((oz, yz, pz), (o1, y1, p1)):
        assert torch.equal(o, o0) and rel_err(y, y0) < 1e-6 and rel_err(p, p0) < 1e-6
    # nothing to fuse: the third string
    g = _seq_func(nn.Linear(64, 64), _MySigmoid(), nn.Linear(64, 64))
    _, _, _, ode = _solve(g, "1", pn_linear_bare=1)
    assert ode.linear_sigmoid == "stock modules (no eligible Linear -> Sigmoid pair)"
    _, _, _, ode = _solve(g, "1")
    assert ode._fwd is None and ode.linear_sigmoid.startswith("stock modules (no eligible pair")
    # -pn_linear_fwd 0 switches the Sigmoid pairs off with the other pairs
    _, _, _, ode = _solve(f, "1", pn_linear_fwd=0)
    assert ode._fwd is None and ode.linear_sigmoid.startswith("stock modules") and _n("fwd_sigmoid") == fwd.n_sigmoid


def test_changing_the_option_between_two_solves_of_one_solver_reinstalls():
    f = _sigmoid_net()
    options.set_option("ts_adapt_type", "none")
    y0 = _y()
    ode = petsc_adjoint.ODEPetsc(backend=SigmoidOps)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    t = torch.tensor([0.0, 0.05], dtype=torch.float64)
    a = ode.odeint_adjoint(y0, t)
    assert ode.linear_sigmoid == "off (-pn_linear_sigmoid 0)" and _n("fwd_sigmoid") == 0
    options.set_option("pn_linear_sigmoid", "1")
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    b = ode.odeint_adjoint(y0, t)
    assert ode.linear_sigmoid.startswith("fused (2 pairs") and _n("fwd_sigmoid") > 0 and torch.equal(a, b)


def test_any_other_value_of_the_option_is_refused():
    f = _sigmoid_net()
    for bad in ("2", "auto", "-1", "yes"):
        with pytest.raises(PnError, match="-pn_linear_sigmoid must be 0 or 1"):
            _solve(f, bad)


def test_the_sigmoid_pairs_of_an_imex_splits_func2_are_counted():
    options.set_option("ts_adapt_type", "none")
    options.set_option("ts_arkimex_type", "3")
    options.set_option("pn_linear_sigmoid", "1")
    fI, fE = DiffusionIM(64, dtype=torch.float32), _sigmoid_net()
    y0 = 0.1 * _y()
    ode = petsc_adjoint.ODEPetsc(backend=SigmoidOps)
    ode.setupTS(y0, fI, step_size=0.05, method="imex", implicit_form=True, imex_form=True, func2=fE, batch_size=256)
    y = y0.clone().requires_grad_(True)
    out = ode.odeint_adjoint(y, torch.tensor([0.0, 0.1], dtype=torch.float64))
    out[-1].pow(2).sum().backward()
    fwd = ode._fwd
    assert fwd is not None and [sorted(p) for _, p in fwd.sigmoid] == [[0, 2]]
    assert fwd.n_sigmoid > 0 and fwd.n_sigmoid_bwd > 0 and _n("fwd_sigmoid") == fwd.n_sigmoid and _n("bwd_sigmoid") == fwd.n_sigmoid_bwd
    assert ode.linear_sigmoid == "fused (2 pairs; %d forward, %d backward calls so far)" % (fwd.n_sigmoid, fwd.n_sigmoid_bwd)
    assert bool(torch.isfinite(y.grad).all()) and bool(torch.isfinite(flat_grads(fE)).all())


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def _last_error(lib):
    return lib.pn_last_error().decode()


def test_the_c_entry_points_take_pn_act_sigmoid_and_still_refuse_3():
    lib = _lib.load()
    assert _lib.PN_ACT_SIGMOID == 4 and (_lib.PN_ACT_IDENTITY, _lib.PN_ACT_TANH, _lib.PN_ACT_RELU) == (0, 1, 2)
    n = 256 * 64
    big = torch.zeros(5 * n + 8)
    g, a, w, gz, dx = (big.data_ptr() + 4 * n * k for k in range(5))
    assert g % 16 == 0
    SIG, PLAIN = _lib.PN_ACT_SIGMOID, _lib.PN_LINEAR_FORM_PLAIN

    def call(pg, pa, pw, pgz, pdx, act=SIG, flags=0, rows=256, dtype=0):
        return lib.pn_linear_bwd_act(None, dtype, rows, 64, 64, pg, pa, pw, act, pgz, pdx, flags)
    ok = (g, a, w, gz, dx)
    for flags in (2, 4, 3, -2):
        assert call(*ok, flags=flags) != 0 and "pn_linear_bwd_act: unknown flag" in _last_error(lib)
    for flags in (0, PLAIN):
        for act in (3, 5, 7, -1):
            assert call(*ok, act=act, flags=flags) != 0
            assert "act is PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID" in _last_error(lib) and "pn_linear_dx" in _last_error(lib)
        # the new value reaches the refusals of every pair: shape, null, alignment, alias
        assert call(*ok, flags=flags, rows=128) != 0 and "pn_linear_bwd: unsupported dtype or shape" in _last_error(lib)
        assert call(*ok, flags=flags, dtype=1) != 0 and "pn_linear_bwd: unsupported dtype or shape" in _last_error(lib)
        for k in range(5):
            assert call(*[None if j == k else p for j, p in enumerate(ok)], flags=flags) != 0 and "null operand" in _last_error(lib)
            assert call(*[p + 4 if j == k else p for j, p in enumerate(ok)], flags=flags) != 0 and "16-byte aligned" in _last_error(lib)
        for alias in (g, a, w, g + 16):
            assert call(g, a, w, alias, dx, flags=flags) != 0 and "gz must not alias g, a or w" in _last_error(lib)
        for alias in (g, a, w, gz, gz + 4 * n - 16):
            assert call(g, a, w, gz, alias, flags=flags) != 0 and "dx must not alias g, a, w or gz" in _last_error(lib)
    # pn_linear_fwd: 3 and 7 are refused by name, 4 goes on to the alias refusal
    p = big.data_ptr()
    for act in (3, 7):
        assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, act, p) != 0
        assert "pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID" in _last_error(lib)
    assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, SIG, p) != 0 and "y must not alias" in _last_error(lib)
    assert not bool(big.any())
