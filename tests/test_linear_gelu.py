"""func's nn.Linear -> nn.GELU pairs (pnode_amd/_linearfwd.py, ``-pn_linear_gelu 0|1``), the pairs that save their PRE-activation: which
children are such a pair, that the default changes nothing, which of the two forward forms an evaluation takes, what every other case
falls back to, the self-checks of their own with their absolute terms, and the C entry points' refusals.  Host logic: ``pn_linear_fwd``
with ``PN_ACT_GELU``, ``pn_linear_fwd_pre`` and ``pn_linear_bwd_act`` are stood in for by the torch expressions they replace
(``F.gelu(F.linear)``; ``gelu_backward`` and ``matmul``: tests/_cpu_linear_gelu.py), so every output must EQUAL the stock modules' and
every gradient agrees with autograd's to 1e-6 in the relative 2-norm (one sum formed by ``mm`` here and by ``addmm`` /
``linear_backward`` there: the bar of tests/test_linear_bare.py)."""
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _cpu_linear_gelu import GeluOps, NoGeluOps
from pnode_amd import _funcguard, _lib, _linearfwd, options, petsc_adjoint
from pnode_amd._lib import PnError
from problems import DiffusionIM, flat_grads, rel_err


class WrongForwardOps(GeluOps):
    def linear_act_fwd(self, x, w, b, act, y=None, z=None, flags=None):
        return super().linear_act_fwd(x, w, b, act, z=z) + (1e-3 if act == "gelu" else 0.0)


class WrongPreOps(GeluOps):
    """The right y beside a pre-activation that is off by 1e-3."""
    def linear_act_fwd(self, x, w, b, act, y=None, z=None, flags=None):
        out = super().linear_act_fwd(x, w, b, act, z=z)
        if z is not None:
            z += 1e-3
        return out


def _bar(g):
    return 32.0 * 2.0 ** -24 * g.abs()             # (the engine's expression, in fp32 as there)


class WrongGzOps(GeluOps):
    """g_z of a GELU pair with one element ONE bit beyond the bar 32 * 2^-24 |g| (and dx of the right g_z)."""
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        if act == "gelu":
            gz = gz.clone()
            i = int(g.reshape(-1).abs().argmax())
            right, bar = gz.view(-1)[i].clone(), _bar(g.reshape(-1)[i])
            v = right + bar
            while bool((v - right).abs() <= bar):
                v = torch.nextafter(v, torch.tensor(float("inf")))
            assert bool((torch.nextafter(v, torch.tensor(-float("inf"))) - right).abs() <= bar)
            gz.view(-1)[i] = v
        return gz, dx


class GzAtTheBarOps(GeluOps):
    """... and with EVERY element moved as far as the bar lets it: no miss."""
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        if act == "gelu":
            v = gz + _bar(g)
            v = torch.where((v - gz).abs() <= _bar(g), v, torch.nextafter(v, torch.full_like(v, -float("inf"))))
            assert bool(((v - gz).abs() <= _bar(g)).all()) and not torch.equal(v, gz)
            gz = v
        return gz, dx


class WrongDxOps(GeluOps):
    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        return gz, dx * (1.001 if act == "gelu" else 1.0)


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self, ops=GeluOps):
        self._ops = ops(torch.device("cpu"), torch.float32, 256 * 64)


@pytest.fixture(autouse=True)
def _host_rules(monkeypatch):
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    NoGeluOps.calls = {}
    options.clear()
    yield
    options.clear()


def _n(what):
    return NoGeluOps.calls.get(what, 0)


def _fwd(f, gelu="1", mode="auto", bwd_mode="auto", bare="0", relu="0", sigmoid="0", ops=GeluOps):
    ode = _Ode(ops)
    fwd = _linearfwd.LinearFwd(ode)
    fwd.keep = ode                                # (LinearFwd holds its solver weakly)
    if gelu is None:
        on = fwd.install(f, list(f.parameters()), mode, bwd_mode, bare, relu, sigmoid)
    else:
        on = fwd.install(f, list(f.parameters()), mode, bwd_mode, bare, relu, sigmoid, gelu_mode=gelu)
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


def _gelu_net(d=64):
    """The func of the GPU solve test: two GELU pairs and a bare head (ROBER's shape: nn.Linear, nn.GELU, ..., nn.Linear)."""
    return _seq_func(nn.Linear(d, d), nn.GELU(), nn.Linear(d, d), nn.GELU(), nn.Linear(d, d))


def _mixed_net(d=64):
    return _seq_func(nn.Linear(d, d), nn.ReLU(), nn.Linear(d, d), nn.Sigmoid(), nn.Linear(d, d), nn.GELU(), nn.Linear(d, d), nn.Tanh(),
                     nn.Linear(d, d))


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


class _MyGelu(nn.GELU):
    pass


def _plan(found):
    return [(type(s), {i: tuple(type(m) for m in p) if isinstance(p, tuple) else type(p) for i, p in d.items()}) for s, d in found]


# ------------------------------------------------------------------------------------------------------------------ finding the pairs
def test_with_gelu_a_linear_gelu_is_a_pair_and_not_a_bare_layer():
    f = _seq_func(nn.Linear(64, 128), nn.GELU(), nn.Linear(128, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), gelu=True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.GELU)})] and refused == {}
    assert plans[0][1][0] == (f.net[0], f.net[1])
    assert _plan(bare) == [(nn.Sequential, {2: nn.Linear})]
    # the other kinds beside it are found as before, each under its own keyword
    f = _mixed_net()
    params = list(f.parameters())
    plans, refused, bare = _linearfwd.find_layers(f, params, True, sigmoid=True, gelu=True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.ReLU), 2: (nn.Linear, nn.Sigmoid), 4: (nn.Linear, nn.GELU),
                                             6: (nn.Linear, nn.Tanh)})] and refused == {}
    assert _plan(bare) == [(nn.Sequential, {8: nn.Linear})]
    plans, _, bare = _linearfwd.find_layers(f, params, gelu=True)
    assert _plan(plans) == [(nn.Sequential, {4: (nn.Linear, nn.GELU), 6: (nn.Linear, nn.Tanh)})]
    assert _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear, 8: nn.Linear})]
    fwd, _, on = _fwd(f, "1", relu="1", sigmoid="1")
    assert on and [sorted(p) for _, p in fwd.plans] == [[6]] and [sorted(p) for _, p in fwd.relu] == [[0]]
    assert [sorted(p) for _, p in fwd.sigmoid] == [[2]] and [sorted(p) for _, p in fwd.gelu.plans] == [[4]] and fwd.gelu_active


def test_a_subclass_of_gelu_is_no_pair():
    f = _seq_func(nn.Linear(64, 64), _MyGelu(), nn.Linear(64, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), gelu=True)
    assert plans == [] and refused == {("Sequential", "GELU"): "a subclass of nn.Linear or nn.GELU"}
    assert _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear})]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fwd, _, on = _fwd(f, "1", mode="1")
        y = _y()
        for _ in range(2):
            with fwd.window():
                got = f(0.0, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_fwd 1: a Linear -> GELU pair" in str(c.message)]
    assert len(msgs) == 1 and "runs the stock modules" in msgs[0], [str(c.message) for c in caught]
    assert not on and fwd.gelu.plans == [] and NoGeluOps.calls == {} and fwd.n_gelu == 0
    assert fwd.gelu_status == "stock modules (no eligible Linear -> GELU pair: a subclass of nn.Linear or nn.GELU)"
    assert torch.equal(got, f(0.0, y))


def test_a_tanh_approximated_gelu_is_no_pair_and_the_status_says_why():
    f = _seq_func(nn.Linear(64, 64), nn.GELU(approximate="tanh"), nn.Linear(64, 64), nn.GELU(), nn.Linear(64, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), gelu=True)
    assert _plan(plans) == [(nn.Sequential, {2: (nn.Linear, nn.GELU)})] and list(refused) == [("Sequential", "GELU")]
    assert "approximate='tanh'" in refused[("Sequential", "GELU")] and "approximate='none'" in refused[("Sequential", "GELU")]
    assert _plan(bare) == [(nn.Sequential, {0: nn.Linear, 4: nn.Linear})]           # its Linear: a bare layer (or a stock module)
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, "1", bare="1")
    got, gg = _eval(f, fwd, y)
    assert on and fwd.n_gelu == 1 and fwd.n_bare == 2 and NoGeluOps.calls == {"fwd_gelu_pre": 1, "fwd_identity": 2, "bwd_gelu": 1, "dx": 2}
    assert torch.equal(got, want) and _close(gg, gw)
    # alone in its container: no pair at all, and the reason is in the status
    g = _seq_func(nn.Linear(64, 64), nn.GELU(approximate="tanh"), nn.Linear(64, 64))
    fwd, _, on = _fwd(g, "1")
    assert not on and fwd.gelu.plans == []
    assert fwd.gelu_status.startswith("stock modules (no eligible Linear -> GELU pair: nn.GELU(approximate='tanh')")
    NoGeluOps.calls = {}
    with fwd.window():
        got = g(0.0, _y())
    assert NoGeluOps.calls == {} and torch.equal(got, g(0.0, _y()))


@pytest.mark.parametrize("where", ["linear", "gelu", "container", "pre", "backward"])
def test_a_user_hook_on_the_pair_or_its_container_runs_the_stock_modules(where):
    f = _gelu_net()
    fwd, _, on = _fwd(f, "1", mode="1")
    assert on and [sorted(p) for _, p in fwd.gelu.plans] == [[0, 2]]
    before = _funcguard.snapshot([f])
    seen = []
    if where == "pre":
        h = f.net[0].register_forward_pre_hook(lambda m, i: seen.append("pre"))
    elif where == "backward":
        h = f.net[1].register_full_backward_hook(lambda m, gi, go: None)
    else:
        m = {"linear": f.net[0], "gelu": f.net[3], "container": f.net}[where]
        h = m.register_forward_hook(lambda m, i, o: seen.append(where))
    y = _y()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):
            with fwd.window():
                assert "forward" not in f.net.__dict__
                got = f(0.0, y)
    msgs = [str(c.message) for c in caught if "a Linear -> GELU pair runs the stock modules" in str(c.message)]
    assert len(msgs) == 1 and "hook on the pair or its container" in msgs[0]
    assert NoGeluOps.calls == {} and torch.equal(got, f(0.0, y))
    if where != "backward":
        assert seen
    h.remove()
    assert _funcguard.snapshot([f]) == before
    with fwd.window():
        f(0.0, y)
    assert NoGeluOps.calls == {"fwd_gelu_pre": 2} and fwd.n_gelu == 2


def test_with_0_or_absent_plans_bare_layers_and_outputs_are_what_they_are_today():
    f = _gelu_net()
    params = list(f.parameters())
    for args, kw in (((), {}), ((False,), {}), ((True,), {"sigmoid": True}), ((), {"gelu": False})):
        plans, refused, bare = _linearfwd.find_layers(f, params, *args, **kw)
        assert plans == [] and refused == {} and _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear, 4: nn.Linear})]
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for gelu in (None, "0"):
        fwd, _, on = _fwd(f, gelu)
        assert not on and not fwd.active and fwd.gelu.plans == [] and fwd.gelu_status == "off (-pn_linear_gelu 0)"
        got, gg = _eval(f, fwd, y)
        assert NoGeluOps.calls == {} and torch.equal(got, want) and _close(gg, gw)
    # under -pn_linear_bare 1 a Linear in front of a GELU is a bare layer
    for gelu in (None, "0"):
        NoGeluOps.calls = {}
        fwd, _, on = _fwd(f, gelu, bare="1")
        assert on and [sorted(b) for _, b in fwd.bare] == [[0, 2, 4]] and fwd.gelu.plans == [] and not fwd.gelu_active
        got, gg = _eval(f, fwd, y)
        assert NoGeluOps.calls == {"fwd_identity": 3, "dx": 3} and fwd.n_gelu == 0 and fwd.n_gelu_bwd == 0
        assert torch.equal(got, want) and _close(gg, gw)


def test_a_call_time_refusal_runs_the_stock_modules_and_its_reason_is_in_the_status():
    f = _gelu_net()
    fwd, _, _ = _fwd(f, "1")
    before = _funcguard.snapshot([f])
    with fwd.window():
        got = f(0.0, _y(rows=128))                # outside pn_linear_fwd_supported
    assert NoGeluOps.calls == {} and torch.equal(got, f.net(_y(rows=128))) and _funcguard.snapshot([f]) == before
    assert fwd.gelu_status == ("fused (2 pairs; 0 forward, 0 backward calls so far; the stock modules where a call is refused, last: "
                               "outside pn_linear_fwd_supported)")
    with fwd.window():
        f(0.0, _y())
    assert NoGeluOps.calls == {"fwd_gelu_pre": 2} and fwd.gelu_status.startswith("fused (2 pairs; 2 forward, 0 backward calls so far;")


# ------------------------------------------------------------------------------------------------------------------- running the pairs
@pytest.mark.parametrize("bare", ["0", "1"])
def test_output_and_gradients_are_the_stock_modules_and_the_counters_are_the_gelu_pairs_own(bare):
    f = _gelu_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, "1", bare=bare)
    assert on and fwd.active and fwd.plans == [] and fwd.relu == [] and fwd.sigmoid == [] and [sorted(p) for _, p in fwd.gelu.plans] == [[0, 2]]
    assert [sorted(b) for _, b in fwd.bare] == [[4]]
    got, gg = _eval(f, fwd, y)
    assert torch.equal(got, want) and _close(gg, gw)
    assert torch.equal(gg[0], gw[0])              # dL/dy: gelu_backward and matmul on both sides
    assert fwd.n_gelu == 2 and fwd.gelu.n_pre == 2 and fwd.gelu.n_y == 0 and fwd.n_gelu_bwd == 2
    assert fwd.n_fused == 0 and fwd.n_fused_bwd == 0 and fwd.n_relu == 0 and fwd.n_relu_bwd == 0 and fwd.n_sigmoid == 0
    assert _n("fwd_gelu_pre") == 2 and _n("fwd_gelu") == 0 and _n("bwd_gelu") == 2 and _n("fwd_tanh") == 0 and _n("bwd_tanh") == 0
    assert (fwd.n_bare, _n("fwd_identity"), _n("dx")) == ((1, 1, 1) if bare == "1" else (0, 0, 0))
    assert fwd.gelu.checked and fwd.gelu.bwd_checked and not fwd.gelu.disabled and not fwd.gelu.bwd_disabled
    assert fwd.gelu_status == "fused (2 pairs; 2 forward, 2 backward calls so far)"
    assert "forward" not in f.net.__dict__
    f(0.0, y)                                     # outside the window: the stock modules
    assert _n("fwd_gelu_pre") == 2


def test_the_pair_saves_x_w_and_the_pre_activation_and_not_its_output():
    f = _seq_func(nn.Linear(64, 64), nn.GELU())
    y = _y().requires_grad_(True)
    fwd, _, _ = _fwd(f, "1")
    with fwd.window():
        out = f(0.0, y)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[0].data_ptr() == y.data_ptr() and saved[1].data_ptr() == f.net[0].weight.data_ptr()
    assert torch.equal(saved[2], F.linear(y, f.net[0].weight, f.net[0].bias)) and not torch.equal(saved[2], out.detach())
    assert all(s.data_ptr() != out.data_ptr() for s in saved)


def test_an_evaluation_nobody_differentiates_takes_the_y_only_form_and_saves_no_pre_activation():
    f = _gelu_net()
    fwd, _, _ = _fwd(f, "1")
    y = _y()
    want = f(0.0, y).detach()
    # grad mode off
    with torch.no_grad(), fwd.window():
        got = f(0.0, y)
    assert torch.equal(got, want) and got.grad_fn is None
    assert NoGeluOps.calls == {"fwd_gelu": 2} and (fwd.n_gelu, fwd.gelu.n_y, fwd.gelu.n_pre) == (2, 2, 0)
    # no input and no parameter requires a gradient
    for p in f.parameters():
        p.requires_grad_(False)
    try:
        with fwd.window():
            got = f(0.0, y)
    finally:
        for p in f.parameters():
            p.requires_grad_(True)
    assert torch.equal(got, want) and got.grad_fn is None
    assert NoGeluOps.calls == {"fwd_gelu": 4} and (fwd.n_gelu, fwd.gelu.n_y, fwd.gelu.n_pre) == (4, 4, 0)
    # ... and the one somebody will: the form with z
    with fwd.window():
        got = f(0.0, y)
    assert got.grad_fn is not None and torch.equal(got.detach(), want)
    assert NoGeluOps.calls == {"fwd_gelu": 4, "fwd_gelu_pre": 2} and (fwd.n_gelu, fwd.gelu.n_y, fwd.gelu.n_pre) == (6, 4, 2)
    assert fwd.gelu_status == "fused (2 pairs; 6 forward, 0 backward calls so far)"


def test_a_mixed_net_counts_each_kind_once_per_evaluation_and_the_head_is_bare():
    f = _mixed_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, "1", bare="1", relu="1", sigmoid="1")
    assert on and [sorted(b) for _, b in fwd.bare] == [[8]]
    for k in (1, 2):
        got, gg = _eval(f, fwd, y)
        assert torch.equal(got, want) and _close(gg, gw)
        assert (fwd.n_fused, fwd.n_relu, fwd.n_sigmoid, fwd.n_gelu, fwd.n_bare) == (k, k, k, k, k)
        assert (fwd.n_fused_bwd, fwd.n_relu_bwd, fwd.n_sigmoid_bwd, fwd.n_gelu_bwd, fwd.n_bare_bwd) == (k, k, k, k, k)
        assert NoGeluOps.calls == {"fwd_relu": k, "fwd_sigmoid": k, "fwd_gelu_pre": k, "fwd_tanh": k, "fwd_identity": k,
                                   "bwd_relu": k, "bwd_sigmoid": k, "bwd_gelu": k, "bwd_tanh": k, "dx": k}
    assert fwd.gelu_status == "fused (1 pairs; 2 forward, 2 backward calls so far)"
    assert fwd.sigmoid_status == "fused (1 pairs; 2 forward, 2 backward calls so far)"
    assert fwd.relu_status == "fused (1 pairs; 2 forward, 2 backward calls so far)"


def test_option_bwd_0_and_a_backend_without_linear_gelu_run_gelu_backward_and_matmul():
    f = _gelu_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for kw in ({"bwd_mode": "0"}, {"ops": NoGeluOps}):
        NoGeluOps.calls = {}
        fwd, _, _ = _fwd(f, "1", **kw)
        got, gg = _eval(f, fwd, y)
        assert fwd.n_gelu == 2 and _n("fwd_gelu_pre") == 2 and fwd.n_gelu_bwd == 0 and _n("bwd_gelu") == 0
        assert torch.equal(got, want) and torch.equal(gg[0], gw[0]) and _close(gg, gw)
    # -pn_linear_bwd 1 says why, once, in the wording of a tanh pair
    fwd, _, _ = _fwd(f, "1", bwd_mode="1", ops=NoGeluOps)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_bwd 1" in str(c.message)]
    assert msgs == ["pnode_amd: -pn_linear_bwd 1: the backward of a Linear -> GELU pair runs the torch operations: "
                    "the backend has no linear_gelu"]


# ---------------------------------------------------------------------------------------------------------------------- the self-checks
def _others_untouched(fwd, k=2):
    """The tanh, ReLU and Sigmoid pairs of the mixed net stay fused, forward and backward."""
    assert not fwd.disabled and not fwd.bwd_disabled and fwd.n_fused == k and fwd.n_fused_bwd == k
    assert not fwd.relu_disabled and not fwd.relu_bwd_disabled and fwd.n_relu == k and fwd.n_relu_bwd == k and fwd.active
    assert not fwd.sig.disabled and not fwd.sig.bwd_disabled and fwd.n_sigmoid == k and fwd.n_sigmoid_bwd == k


@pytest.mark.parametrize("ops,what", [(WrongForwardOps, "pn_linear_fwd and F.gelu(F.linear) differ by"),
                                      (WrongPreOps, "the pre-activation of pn_linear_fwd_pre and F.linear differ by")])
def test_a_gelu_forward_off_by_a_thousandth_switches_off_the_gelu_pairs_only(ops, what):
    f = _mixed_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, ode, _ = _fwd(f, "1", relu="1", sigmoid="1", ops=ops)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        got2, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> GELU forward is switched off" in str(c.message)]
    assert len(msgs) == 1 and what in msgs[0]
    assert fwd.gelu.disabled and fwd.n_gelu == 0 and _n("fwd_gelu_pre") == 1 and not fwd.gelu_active
    assert fwd.gelu_status.startswith("stock modules (" + what)
    _others_untouched(fwd)
    assert torch.equal(got, want) and torch.equal(got2, want) and _close(g1, gw) and _close(g2, gw)


@pytest.mark.parametrize("ops,what", [(WrongGzOps, "g_z by more than 32 * 2^-24 |g|"), (WrongDxOps, "dx by")])
def test_a_wrong_gelu_backward_switches_off_the_gelu_backward_only(ops, what):
    f = _mixed_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, "1", relu="1", sigmoid="1", ops=ops)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        _, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> GELU backward is switched off" in str(c.message)]
    assert len(msgs) == 1 and what in msgs[0]
    assert fwd.gelu.bwd_disabled and fwd.n_gelu_bwd == 0 and _n("bwd_gelu") == 1 and what in fwd.gelu.bwd_why
    assert "pn_linear_bwd_act and gelu_backward + matmul differ" in fwd.gelu.bwd_why
    # the GELU forward stays fused
    assert not fwd.gelu.disabled and fwd.n_gelu == 2 and fwd.gelu_status == "fused (1 pairs; 2 forward, 0 backward calls so far)"
    _others_untouched(fwd)
    assert torch.equal(got, want) and _close(g1, gw) and _close(g2, gw)


def test_a_g_z_moved_as_far_as_the_bar_lets_it_is_no_miss():
    f = _gelu_net()
    y = _y().requires_grad_(True)
    fwd, _, _ = _fwd(f, "1", ops=GzAtTheBarOps)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _eval(f, fwd, y)
    assert fwd.gelu.bwd_checked and not fwd.gelu.bwd_disabled and fwd.n_gelu_bwd == 2


def test_pre_activations_of_zero_and_at_the_zero_of_the_derivative_do_not_trip_the_checks():
    """Rows with z = 0 exactly (x = 0, b = 0: the scale of the forward's bar is 0 and GELU's value an exact 0) and rows with
    z = -0.7518 (the zero of GELU's derivative: g_z is about 0 whatever g is -- a bar relative to |g_z| would be empty)."""
    f = _seq_func(nn.Linear(64, 64), nn.GELU(), nn.Linear(64, 64))
    with torch.no_grad():
        f.net[0].bias.zero_()
    y = _y()
    y[::3] = 0.0                                  # rows of scale 0: z = 0
    with torch.no_grad():                         # rows whose z is -0.7518 in every column: x = 0 but for a bias fed through column 0
        f.net[0].weight[:, 0] = -0.7518
    y[1::3] = 0.0
    y[1::3, 0] = 1.0
    y.requires_grad_(True)
    with torch.no_grad():
        z = F.linear(y, f.net[0].weight, f.net[0].bias)
        d = torch.ops.aten.gelu_backward(torch.ones_like(z), z, approximate="none")
    assert bool((z[::3] == 0).all()) and bool((z[1::3] == -0.7518).all()) and float(d[1::3].abs().max()) < 1e-4
    want, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, "1")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got, gg = _eval(f, fwd, y)
    assert fwd.gelu.checked and not fwd.gelu.disabled and fwd.gelu.bwd_checked and not fwd.gelu.bwd_disabled
    assert fwd.n_gelu == 1 and fwd.n_gelu_bwd == 1 and torch.equal(got, want) and _close(gg, gw)
    # ... and without a bias at all
    g = _seq_func(nn.Linear(64, 64, bias=False), nn.GELU())
    fwd, _, _ = _fwd(g, "1")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _eval(g, fwd, y)
    assert not fwd.gelu.disabled and not fwd.gelu.bwd_disabled and fwd.n_gelu == 1 and fwd.n_gelu_bwd == 1


# --------------------------------------------------------------------------------------------------------------- solves and the option
def _solve(f, gelu, backend=GeluOps, steps=3, **more):
    options.clear()
    options.set_option("ts_adapt_type", "none")
    if gelu is not None:
        options.set_option("pn_linear_gelu", gelu)
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
    f = _gelu_net()
    o0, y0, p0, ode0 = _solve(f, None)
    assert ode0._fwd is None and ode0.linear_gelu == "off (-pn_linear_gelu 0)" and NoGeluOps.calls == {}
    oz, yz, pz, odez = _solve(f, "0", pn_linear_bare=1)
    assert odez.linear_gelu == "off (-pn_linear_gelu 0)" and odez._fwd.n_gelu == 0 and odez._fwd.n_bare > 0 and _n("fwd_gelu") == 0
    o1, y1, p1, ode1 = _solve(f, "1", pn_linear_bare=1)
    fwd = ode1._fwd
    # rk4 x 3 steps: at least four stage evaluations and four stage VJPs per step, two GELU pairs each
    assert fwd.n_gelu >= 3 * 4 * 2 * 2 and fwd.n_gelu_bwd >= 3 * 4 * 2 and fwd.n_fused == 0 and fwd.n_relu == 0 and fwd.n_sigmoid == 0
    assert 2 * fwd.n_bare == fwd.n_gelu and 2 * fwd.n_bare_bwd == fwd.n_gelu_bwd
    # the forward sweep keeps no tapes: y alone; the stage VJPs of the reverse sweep: y and z, at least one backward each
    assert fwd.gelu.n_y >= 3 * 4 * 2 and fwd.gelu.n_pre >= 3 * 4 * 2 and fwd.n_gelu_bwd >= fwd.gelu.n_pre
    assert (_n("fwd_gelu"), _n("fwd_gelu_pre"), _n("bwd_gelu")) == (fwd.gelu.n_y, fwd.gelu.n_pre, fwd.n_gelu_bwd)
    assert ode1.linear_gelu == "fused (2 pairs; %d forward, %d backward calls so far)" % (fwd.n_gelu, fwd.n_gelu_bwd)
    assert ode1.linear_bare.startswith("fused (1 layers") and ode1.linear_fwd.startswith("stock modules")
    assert ode1.linear_relu == "off (-pn_linear_relu 0)" and ode1.linear_sigmoid == "off (-pn_linear_sigmoid 0)"
    assert ode1.linear_param_grads.startswith("engine") and ode1._lin.n_autograd == 0 and ode1._lin.n_clean > 0
    for o, y, p in ((oz, yz, pz), (o1, y1, p1)):
        assert torch.equal(o, o0) and rel_err(y, y0) < 1e-6 and rel_err(p, p0) < 1e-6
    # nothing to fuse: the third string
    g = _seq_func(nn.Linear(64, 64), _MyGelu(), nn.Linear(64, 64))
    _, _, _, ode = _solve(g, "1", pn_linear_bare=1)
    assert ode.linear_gelu == "stock modules (no eligible Linear -> GELU pair: a subclass of nn.Linear or nn.GELU)"
    _, _, _, ode = _solve(g, "1")
    assert ode._fwd is None and ode.linear_gelu.startswith("stock modules (no eligible pair")
    # -pn_linear_fwd 0 switches the GELU pairs off with the other pairs
    _, _, _, ode = _solve(f, "1", pn_linear_fwd=0)
    assert ode._fwd is None and ode.linear_gelu.startswith("stock modules") and _n("fwd_gelu") + _n("fwd_gelu_pre") == fwd.n_gelu


def test_changing_the_option_between_two_solves_of_one_solver_reinstalls():
    f = _gelu_net()
    options.set_option("ts_adapt_type", "none")
    y0 = _y()
    ode = petsc_adjoint.ODEPetsc(backend=GeluOps)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    t = torch.tensor([0.0, 0.05], dtype=torch.float64)
    a = ode.odeint_adjoint(y0, t)
    assert ode.linear_gelu == "off (-pn_linear_gelu 0)" and _n("fwd_gelu") == 0 and _n("fwd_gelu_pre") == 0
    options.set_option("pn_linear_gelu", "1")
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    b = ode.odeint_adjoint(y0, t)
    assert ode.linear_gelu.startswith("fused (2 pairs") and _n("fwd_gelu") + _n("fwd_gelu_pre") > 0 and torch.equal(a, b)


def test_any_other_value_of_the_option_is_refused():
    f = _gelu_net()
    for bad in ("2", "auto", "-1", "yes"):
        with pytest.raises(PnError, match="-pn_linear_gelu must be 0 or 1"):
            _solve(f, bad)


def test_the_gelu_pairs_of_an_imex_splits_func2_are_counted():
    options.set_option("ts_adapt_type", "none")
    options.set_option("ts_arkimex_type", "3")
    options.set_option("pn_linear_gelu", "1")
    fI, fE = DiffusionIM(64, dtype=torch.float32), _gelu_net()
    y0 = 0.1 * _y()
    ode = petsc_adjoint.ODEPetsc(backend=GeluOps)
    ode.setupTS(y0, fI, step_size=0.05, method="imex", implicit_form=True, imex_form=True, func2=fE, batch_size=256)
    y = y0.clone().requires_grad_(True)
    out = ode.odeint_adjoint(y, torch.tensor([0.0, 0.1], dtype=torch.float64))
    out[-1].pow(2).sum().backward()
    fwd = ode._fwd
    assert fwd is not None and [sorted(p) for _, p in fwd.gelu.plans] == [[0, 2]]
    assert fwd.n_gelu > 0 and fwd.n_gelu_bwd > 0 and _n("fwd_gelu") + _n("fwd_gelu_pre") == fwd.n_gelu and _n("bwd_gelu") == fwd.n_gelu_bwd
    assert ode.linear_gelu == "fused (2 pairs; %d forward, %d backward calls so far)" % (fwd.n_gelu, fwd.n_gelu_bwd)
    assert bool(torch.isfinite(y.grad).all()) and bool(torch.isfinite(flat_grads(fE)).all())


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def _last_error(lib):
    return lib.pn_last_error().decode()


def test_the_c_entry_points_take_pn_act_gelu_and_still_refuse_3_5_7():
    lib = _lib.load()
    assert _lib.PN_ACT_GELU == 8 and _lib.PN_ACT_SIGMOID == 4 and (_lib.PN_ACT_IDENTITY, _lib.PN_ACT_TANH, _lib.PN_ACT_RELU) == (0, 1, 2)
    assert _lib.PN_ABI_VERSION == 4 and lib.pn_abi_version() == 4
    n = 256 * 64
    big = torch.zeros(5 * n + 8)
    g, a, w, gz, dx = (big.data_ptr() + 4 * n * k for k in range(5))
    assert g % 16 == 0
    GELU, PLAIN = _lib.PN_ACT_GELU, _lib.PN_LINEAR_FORM_PLAIN

    def call(pg, pa, pw, pgz, pdx, act=GELU, flags=0, rows=256, dtype=0):
        return lib.pn_linear_bwd_act(None, dtype, rows, 64, 64, pg, pa, pw, act, pgz, pdx, flags)
    ok = (g, a, w, gz, dx)
    for flags in (2, 4, 3, -2):
        assert call(*ok, flags=flags) != 0 and "pn_linear_bwd_act: unknown flag" in _last_error(lib)
    for flags in (0, PLAIN):
        for act in (3, 5, 7, -1):
            assert call(*ok, act=act, flags=flags) != 0
            assert "act is PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU" in _last_error(lib) and "pn_linear_dx" in _last_error(lib)
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
    # pn_linear_fwd / pn_linear_fwd_form: 3, 5, 7 and -1 are refused by name, 8 goes on to the alias refusal
    p = big.data_ptr()
    for act in (3, 5, 7, -1):
        assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, act, p) != 0
        assert "pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU" in _last_error(lib)
    assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, GELU, p) != 0 and "y must not alias" in _last_error(lib)
    assert lib.pn_linear_fwd_form(None, 0, 256, 64, 64, p, p, None, GELU, p, PLAIN) != 0 and "y must not alias" in _last_error(lib)
    assert not bool(big.any())


def test_pn_linear_fwd_pre_refuses_a_bad_z_a_bad_flag_shape_dtype_and_act_and_writes_nothing():
    lib = _lib.load()
    rows, out_f, in_f = 256, 64, 64
    n = rows * out_f                              # (x, y and z: rows x 64; w: 64 x 64 and b: 64 inside one slot of n floats each)
    big = torch.zeros(5 * n + 8)
    x, w, b, y, z = (big.data_ptr() + 4 * n * k for k in range(5))
    assert x % 16 == 0
    GELU, PLAIN = _lib.PN_ACT_GELU, _lib.PN_LINEAR_FORM_PLAIN

    def call(px=x, pw=w, pb=b, py=y, pz=z, act=GELU, flags=0, rows=rows, dtype=0):
        return lib.pn_linear_fwd_pre(None, dtype, rows, out_f, in_f, px, pw, pb, act, py, pz, flags)
    for flags in (0, PLAIN):
        assert call(pz=None, flags=flags) != 0 and "pn_linear_fwd_pre: z is null" in _last_error(lib)
        for off in (4, 8, 12):
            assert call(pz=z + off, flags=flags) != 0 and "pn_linear_fwd_pre: z must be 16-byte aligned" in _last_error(lib)
        for alias in (y, y + 4 * n - 16, x, x + 16, w, w + 4 * out_f * in_f - 16, b, b + 4 * out_f - 16):
            assert call(pz=alias, flags=flags) != 0 and "pn_linear_fwd_pre: z must not alias y, x, w or b" in _last_error(lib), alias
        # (the first 16 bytes behind b's out_f values are nobody's)
        assert call(px=None, flags=flags) != 0 and "null operand" in _last_error(lib)
        assert call(py=x, flags=flags) != 0 and "y must not alias" in _last_error(lib)
        assert call(rows=128, flags=flags) != 0 and "pn_linear_fwd: unsupported dtype or shape" in _last_error(lib)
        assert call(dtype=1, flags=flags) != 0 and "pn_linear_fwd: unsupported dtype or shape" in _last_error(lib)
        for act in (3, 5, 7, -1):
            assert call(act=act, flags=flags) != 0
            assert "pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID" in _last_error(lib)
    for flags in (2, 4, 3, -2):
        assert call(flags=flags) != 0 and "pn_linear_fwd_pre: unknown flag" in _last_error(lib)
    assert not bool(big.any())
