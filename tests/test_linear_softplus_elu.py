"""func's nn.Linear -> nn.Softplus and nn.Linear -> nn.ELU pairs (pnode_amd/_linearfwd.py, ``-pn_linear_softplus 0|1``,
``-pn_linear_elu 0|1``): which children are such a pair and which parameters make none, that the default changes nothing, the statuses,
the counters, the self-checks of their own, what ``-pn_linear_bwd 0`` and ``-pn_linear_fwd 0`` fall back to, a solve per act, and the C
entry points' refusals.  Host logic: the kernels are stood in for by their four formulas spelled in torch
(tests/_cpu_linear_softplus_elu.py).  These are the kernels' formulas, not aten's kernels (``F.elu`` forms ``exp(z) - 1``), so outputs
and gradients agree with the stock modules' to 1e-6 in the relative 2-norm -- a few ulp of values of size one -- and not bit for bit."""
import warnings

import pytest
import torch
import torch.nn as nn

from _cpu_linear_gelu import NoGeluOps
from _cpu_linear_softplus_elu import NoSoftplusEluOps, SoftplusEluOps
from pnode_amd import _lib, _linearfwd, options, petsc_adjoint
from pnode_amd._lib import PnError
from problems import flat_grads, rel_err

KINDS = [("softplus", nn.Softplus, "Softplus"), ("elu", nn.ELU, "ELU")]


class WrongForwardOps(SoftplusEluOps):
    wrong = "softplus"

    def linear_act_fwd(self, x, w, b, act, y=None, z=None, flags=None):
        return super().linear_act_fwd(x, w, b, act, z=z) + (1e-3 if act == self.wrong else 0.0)


class WrongEluForwardOps(WrongForwardOps):
    wrong = "elu"


class WrongGzOps(SoftplusEluOps):
    """g_z of one kind with its largest-|g| element moved by 8 * 2^-24 |g|: beyond both bars (4 and 1.5)."""
    wrong = "softplus"

    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        if act == self.wrong:
            gz = gz.clone()
            i = int(g.reshape(-1).abs().argmax())
            gz.view(-1)[i] += 8.0 * 2.0 ** -24 * g.reshape(-1)[i].abs()
        return gz, dx


class WrongEluGzOps(WrongGzOps):
    wrong = "elu"


class WrongDxOps(SoftplusEluOps):
    wrong = "softplus"

    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        gz, dx = super().linear_bwd(g, a, w, act=act)
        return gz, dx * (1.001 if act == self.wrong else 1.0)


class WrongEluDxOps(WrongDxOps):
    wrong = "elu"


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self, ops):
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


def _fwd(f, softplus="1", elu="1", mode="auto", bwd_mode="auto", bare="0", ops=SoftplusEluOps, **more):
    ode = _Ode(ops)
    fwd = _linearfwd.LinearFwd(ode)
    fwd.keep = ode                                # (LinearFwd holds its solver weakly)
    kw = dict(more)
    if softplus is not None:
        kw["softplus_mode"] = softplus
    if elu is not None:
        kw["elu_mode"] = elu
    on = fwd.install(f, list(f.parameters()), mode, bwd_mode, bare, **kw)
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


def _net(cls, d=64):
    return _seq_func(nn.Linear(d, d), cls(), nn.Linear(d, d), cls(), nn.Linear(d, d))


def _both_net(d=64):
    return _seq_func(nn.Linear(d, d), nn.Softplus(), nn.Linear(d, d), nn.ELU(), nn.Linear(d, d))


def _eval(f, fwd, y):
    with fwd.window():
        out = f(0.0, y)
    return out, torch.autograd.grad(out.pow(2).sum(), [y] + list(f.parameters()))


def _stock(f, y):
    out = f(0.0, y)
    return out, torch.autograd.grad(out.pow(2).sum(), [y] + list(f.parameters()))


def _close(gg, gw, tol=1e-6):
    return all(rel_err(a, b) < tol for a, b in zip(gg, gw))


def _plan(found):
    return [(type(s), {i: tuple(type(m) for m in p) if isinstance(p, tuple) else type(p) for i, p in d.items()}) for s, d in found]


class _MySoftplus(nn.Softplus):
    pass


class _MyElu(nn.ELU):
    pass


# ------------------------------------------------------------------------------------------------------------------ finding the pairs
def test_with_the_keywords_the_pairs_are_found_and_without_them_nothing_changes():
    f = _both_net()
    params = list(f.parameters())
    for args, kw in (((), {}), ((True,), {"sigmoid": True, "gelu": True}), ((), {"softplus": False, "elu": False})):
        plans, refused, bare = _linearfwd.find_layers(f, params, *args, **kw)
        assert plans == [] and refused == {} and _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear, 4: nn.Linear})]
    plans, refused, bare = _linearfwd.find_layers(f, params, softplus=True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.Softplus)})] and refused == {}
    assert _plan(bare) == [(nn.Sequential, {2: nn.Linear, 4: nn.Linear})]           # the Linear in front of the ELU: a bare layer
    plans, refused, bare = _linearfwd.find_layers(f, params, elu=True)
    assert _plan(plans) == [(nn.Sequential, {2: (nn.Linear, nn.ELU)})] and _plan(bare) == [(nn.Sequential, {0: nn.Linear, 4: nn.Linear})]
    plans, refused, bare = _linearfwd.find_layers(f, params, softplus=True, elu=True)
    assert _plan(plans) == [(nn.Sequential, {0: (nn.Linear, nn.Softplus), 2: (nn.Linear, nn.ELU)})] and refused == {}
    assert plans[0][1][2] == (f.net[2], f.net[3]) and _plan(bare) == [(nn.Sequential, {4: nn.Linear})]
    fwd, _, on = _fwd(f)
    assert on and [sorted(p) for _, p in fwd.softplus.plans] == [[0]] and [sorted(p) for _, p in fwd.elu.plans] == [[2]]
    assert fwd.plans == [] and fwd.relu == [] and fwd.sigmoid == [] and fwd.gelu.plans == []


def test_other_parameters_make_no_pair_and_the_reason_is_kept():
    f = _seq_func(nn.Linear(64, 64), nn.Softplus(beta=2), nn.Linear(64, 64), nn.Softplus(threshold=10), nn.Linear(64, 64), nn.ELU(alpha=0.5),
                  nn.Linear(64, 64), nn.Softplus(), nn.Linear(64, 64), nn.ELU(inplace=True), nn.Linear(64, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), softplus=True, elu=True)
    assert _plan(plans) == [(nn.Sequential, {6: (nn.Linear, nn.Softplus), 8: (nn.Linear, nn.ELU)})]          # inplace=True is a pair
    assert set(refused) == {("Sequential", "Softplus"), ("Sequential", "ELU")}
    assert "beta=2" in refused[("Sequential", "Softplus")] and "beta == 1 and threshold == 20" in refused[("Sequential", "Softplus")]
    assert "alpha=0.5" in refused[("Sequential", "ELU")] and "alpha == 1" in refused[("Sequential", "ELU")]
    assert _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear, 4: nn.Linear, 10: nn.Linear})]
    g = _seq_func(nn.Linear(64, 64), nn.Softplus(threshold=10), nn.Linear(64, 64))
    _, refused, _ = _linearfwd.find_layers(g, list(g.parameters()), softplus=True)
    assert "threshold=10" in refused[("Sequential", "Softplus")]
    # alone in their container: the reason is in the status, and -pn_linear_fwd 1 warns once per kind
    h = _seq_func(nn.Linear(64, 64), nn.Softplus(beta=2), nn.Linear(64, 64), nn.ELU(alpha=0.5), nn.Linear(64, 64))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fwd, _, on = _fwd(h, mode="1")
    assert not on and fwd.softplus.plans == [] and fwd.elu.plans == []
    assert fwd.softplus_status.startswith("stock modules (no eligible Linear -> Softplus pair: nn.Softplus(beta=2")
    assert fwd.elu_status.startswith("stock modules (no eligible Linear -> ELU pair: nn.ELU(alpha=0.5")
    msgs = [str(c.message) for c in caught]
    assert sum("a Linear -> Softplus pair of Sequential runs the stock modules" in m for m in msgs) == 1
    assert sum("a Linear -> ELU pair of Sequential runs the stock modules" in m for m in msgs) == 1
    y = _y()
    with fwd.window():
        got = h(0.0, y)
    assert NoGeluOps.calls == {} and torch.equal(got, h(0.0, y))


def test_a_subclass_is_no_pair():
    f = _seq_func(nn.Linear(64, 64), _MySoftplus(), nn.Linear(64, 64), _MyElu(), nn.Linear(64, 64))
    plans, refused, bare = _linearfwd.find_layers(f, list(f.parameters()), softplus=True, elu=True)
    assert plans == [] and refused == {("Sequential", "Softplus"): "a subclass of nn.Linear or nn.Softplus",
                                       ("Sequential", "ELU"): "a subclass of nn.Linear or nn.ELU"}
    assert _plan(bare) == [(nn.Sequential, {0: nn.Linear, 2: nn.Linear, 4: nn.Linear})]


@pytest.mark.parametrize("name,cls,label", KINDS)
def test_at_0_such_a_linear_is_a_stock_module_or_a_bare_layer(name, cls, label):
    f = _net(cls)
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for mode in (None, "0"):
        fwd, _, on = _fwd(f, mode, mode)
        assert not on and not fwd.active and getattr(fwd, name).status == "off (-pn_linear_%s 0)" % name
        got, gg = _eval(f, fwd, y)
        assert NoGeluOps.calls == {} and torch.equal(got, want) and _close(gg, gw)
        NoGeluOps.calls = {}
        fwd, _, on = _fwd(f, mode, mode, bare="1")
        assert on and [sorted(b) for _, b in fwd.bare] == [[0, 2, 4]] and getattr(fwd, name).plans == []
        got, gg = _eval(f, fwd, y)
        assert NoGeluOps.calls == {"fwd_identity": 3, "dx": 3} and torch.equal(got, want) and _close(gg, gw)
        NoGeluOps.calls = {}


# ------------------------------------------------------------------------------------------------------------------- running the pairs
@pytest.mark.parametrize("name,cls,label", KINDS)
@pytest.mark.parametrize("bare", ["0", "1"])
def test_output_gradients_counters_and_status(name, cls, label, bare):
    f = _net(cls)
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, bare=bare)
    st = getattr(fwd, name)
    other = fwd.elu if name == "softplus" else fwd.softplus
    assert on and fwd.active and st.active and [sorted(p) for _, p in st.plans] == [[0, 2]] and [sorted(b) for _, b in fwd.bare] == [[4]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got, gg = _eval(f, fwd, y)
    assert rel_err(got, want) < 1e-6 and _close(gg, gw)
    assert (st.n, st.n_bwd, other.n, other.n_bwd) == (2, 2, 0, 0) and st.checked and st.bwd_checked and not st.disabled and not st.bwd_disabled
    assert fwd.n_fused == 0 and fwd.n_relu == 0 and fwd.n_sigmoid == 0 and fwd.n_gelu == 0
    assert _n("fwd_" + name) == 2 and _n("bwd_" + name) == 2 and _n("fwd_tanh") == 0
    assert (fwd.n_bare, _n("fwd_identity"), _n("dx")) == ((1, 1, 1) if bare == "1" else (0, 0, 0))
    assert st.status == "fused (2 pairs; 2 forward, 2 backward calls so far)"
    assert other.status == "stock modules (no eligible Linear -> %s pair)" % other.name
    assert "forward" not in f.net.__dict__
    f(0.0, y)                                     # outside the window: the stock modules
    assert _n("fwd_" + name) == 2


def test_the_pair_saves_its_output_and_an_inplace_elu_is_not_called():
    f = _seq_func(nn.Linear(64, 64), nn.ELU(inplace=True))
    y = _y().requires_grad_(True)
    fwd, _, on = _fwd(f)
    assert on
    with fwd.window():
        out = f(0.0, y)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[0].data_ptr() == y.data_ptr() and saved[2].data_ptr() == out.data_ptr()
    assert fwd.elu.n == 1 and _n("fwd_elu") == 1
    assert bool((out.detach() > -1.0).all()) and bool((out.detach() < 0).any())      # (not run in place on the Linear's result twice)


def test_both_kinds_in_one_net_count_apart_and_a_call_time_refusal_is_in_the_status():
    f = _both_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, bare="1")
    for k in (1, 2):
        got, gg = _eval(f, fwd, y)
        assert rel_err(got, want) < 1e-6 and _close(gg, gw)
        assert (fwd.softplus.n, fwd.elu.n, fwd.n_bare, fwd.softplus.n_bwd, fwd.elu.n_bwd, fwd.n_bare_bwd) == (k,) * 6
        assert NoGeluOps.calls == {"fwd_softplus": k, "fwd_elu": k, "fwd_identity": k, "bwd_softplus": k, "bwd_elu": k, "dx": k}
    small = _y(rows=128)
    with fwd.window():
        got = f(0.0, small)                       # outside pn_linear_fwd_supported
    assert torch.equal(got, f.net(small)) and fwd.softplus.n == 2
    for st in (fwd.softplus, fwd.elu):
        assert st.status == ("fused (1 pairs; 2 forward, 2 backward calls so far; the stock modules where a call is refused, last: "
                             "outside pn_linear_fwd_supported)")


@pytest.mark.parametrize("name,cls,label", KINDS)
def test_a_user_hook_runs_the_stock_modules(name, cls, label):
    f = _net(cls)
    fwd, _, on = _fwd(f, mode="1")
    h = f.net[1].register_forward_hook(lambda m, i, o: None)
    y = _y()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):
            with fwd.window():
                got = f(0.0, y)
    msgs = [str(c.message) for c in caught if "a Linear -> %s pair runs the stock modules" % label in str(c.message)]
    assert len(msgs) == 1 and "hook on the pair or its container" in msgs[0], [str(c.message) for c in caught]
    assert NoGeluOps.calls == {} and torch.equal(got, f(0.0, y))
    h.remove()
    with fwd.window():
        f(0.0, y)
    assert NoGeluOps.calls == {"fwd_" + name: 2}


@pytest.mark.parametrize("name,cls,label", KINDS)
def test_bwd_0_and_a_backend_without_the_capability_run_the_torch_expression_and_matmul(name, cls, label):
    f = _net(cls)
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for kw in ({"bwd_mode": "0"}, {"ops": NoSoftplusEluOps}):
        NoGeluOps.calls = {}
        fwd, _, _ = _fwd(f, **kw)
        st = getattr(fwd, name)
        got, gg = _eval(f, fwd, y)
        assert st.n == 2 and _n("fwd_" + name) == 2 and st.n_bwd == 0 and _n("bwd_" + name) == 0
        assert rel_err(got, want) < 1e-6 and _close(gg, gw)
    fwd, _, _ = _fwd(f, bwd_mode="1", ops=NoSoftplusEluOps)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "-pn_linear_bwd 1" in str(c.message)]
    assert msgs == ["pnode_amd: -pn_linear_bwd 1: the backward of a Linear -> %s pair runs the torch operations: "
                    "the backend has no linear_%s" % (label, name)]


def test_the_torch_expressions_of_bwd_0_are_the_issues():
    g, a = _y(seed=3), torch.nn.functional.softplus(_y(seed=4))
    assert torch.equal(_linearfwd._softplus_gz(g, a), g * (-torch.expm1(-a)))
    e = torch.nn.functional.elu(_y(seed=4))
    assert torch.equal(_linearfwd._elu_gz(g, e), torch.ops.aten.elu_backward(g, 1, 1, 1, True, e))
    assert torch.equal(_linearfwd._elu_gz(g, e)[e > 0], g[e > 0])


# ---------------------------------------------------------------------------------------------------------------------- the self-checks
@pytest.mark.parametrize("ops,name", [(WrongForwardOps, "softplus"), (WrongEluForwardOps, "elu")])
def test_a_forward_off_by_a_thousandth_switches_off_that_kind_only(ops, name):
    f = _both_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, ops=ops)
    st = getattr(fwd, name)
    other = fwd.elu if name == "softplus" else fwd.softplus
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        got2, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> %s forward is switched off" % st.name in str(c.message)]
    assert len(msgs) == 1 and "pn_linear_fwd and %s differ by" % st.torch_fwd in msgs[0]
    assert st.disabled and st.n == 0 and _n("fwd_" + name) == 1 and not st.active
    assert st.status.startswith("stock modules (pn_linear_fwd and %s differ by" % st.torch_fwd)
    assert not other.disabled and not other.bwd_disabled and other.n == 2 and other.n_bwd == 2 and fwd.active
    for got_, g_ in ((got, g1), (got2, g2)):
        assert rel_err(got_, want) < 1e-6 and _close(g_, gw)


@pytest.mark.parametrize("ops,name,what", [(WrongGzOps, "softplus", "g_z by more than 4 * 2^-24 |g|"), (WrongDxOps, "softplus", "dx by"),
                                           (WrongEluGzOps, "elu", "g_z by more than 1.5 * 2^-24 |g|"), (WrongEluDxOps, "elu", "dx by")])
def test_a_wrong_backward_switches_off_that_kinds_backward_only(ops, name, what):
    f = _both_net()
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, ops=ops)
    st = getattr(fwd, name)
    other = fwd.elu if name == "softplus" else fwd.softplus
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got, g1 = _eval(f, fwd, y)
        _, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "Linear -> %s backward is switched off" % st.name in str(c.message)]
    assert len(msgs) == 1 and what in msgs[0]
    assert st.bwd_disabled and st.n_bwd == 0 and _n("bwd_" + name) == 1 and what in st.bwd_why
    assert "pn_linear_bwd_act and %s differ" % st.torch_bwd in st.bwd_why
    assert not st.disabled and st.n == 2 and st.status == "fused (1 pairs; 2 forward, 0 backward calls so far)"
    assert not other.disabled and not other.bwd_disabled and other.n == 2 and other.n_bwd == 2
    assert rel_err(got, want) < 1e-6 and _close(g1, gw) and _close(g2, gw)


def test_rows_of_scale_zero_do_not_trip_the_checks():
    """x = 0 and b = 0: z = 0 exactly, the scale of the forward's bar is 0; Softplus gives log 2 there and ELU an exact 0."""
    for cls in (nn.Softplus, nn.ELU):
        f = _seq_func(nn.Linear(64, 64, bias=False), cls(), nn.Linear(64, 64))
        y = _y()
        y[::3] = 0.0
        y.requires_grad_(True)
        fwd, _, _ = _fwd(f)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _eval(f, fwd, y)
        st = fwd._state(f.net[1])
        assert st.checked and st.bwd_checked and not st.disabled and not st.bwd_disabled and st.n == 1 and st.n_bwd == 1


# --------------------------------------------------------------------------------------------------------------- solves and the options
def _solve(f, backend=SoftplusEluOps, steps=3, **more):
    options.clear()
    options.set_option("ts_adapt_type", "none")
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


@pytest.mark.parametrize("name,cls,label", KINDS)
def test_a_whole_solve_and_the_three_statuses(name, cls, label):
    f = _net(cls)
    opt = "pn_linear_" + name
    status = lambda ode: getattr(ode, "linear_" + name)
    o0, y0, p0, ode0 = _solve(f)
    assert ode0._fwd is None and status(ode0) == "off (-%s 0)" % opt and NoGeluOps.calls == {}
    oz, yz, pz, odez = _solve(f, pn_linear_bare=1, **{opt: "0"})
    assert status(odez) == "off (-%s 0)" % opt and getattr(odez._fwd, name).n == 0 and odez._fwd.n_bare > 0 and _n("fwd_" + name) == 0
    assert torch.equal(oz, o0)
    o1, y1, p1, ode1 = _solve(f, pn_linear_bare=1, **{opt: "1"})
    fwd = ode1._fwd
    st = getattr(fwd, name)
    # rk4 x 3 steps: at least four stage evaluations and four stage VJPs per step, two pairs each
    assert st.n >= 3 * 4 * 2 * 2 and st.n_bwd >= 3 * 4 * 2 and fwd.n_fused == 0 and fwd.n_gelu == 0 and fwd.n_sigmoid == 0
    assert 2 * fwd.n_bare == st.n and 2 * fwd.n_bare_bwd == st.n_bwd
    assert (_n("fwd_" + name), _n("bwd_" + name)) == (st.n, st.n_bwd)
    assert status(ode1) == "fused (2 pairs; %d forward, %d backward calls so far)" % (st.n, st.n_bwd)
    other = "elu" if name == "softplus" else "softplus"
    assert getattr(ode1, "linear_" + other) == "off (-pn_linear_%s 0)" % other
    assert ode1.linear_gelu == "off (-pn_linear_gelu 0)" and ode1.linear_sigmoid == "off (-pn_linear_sigmoid 0)"
    assert ode1.linear_bare.startswith("fused (1 layers") and ode1.linear_param_grads.startswith("engine") and ode1._lin.n_autograd == 0
    assert rel_err(o1, o0) < 1e-6 and rel_err(y1, y0) < 1e-6 and rel_err(p1, p0) < 1e-6
    # nothing to fuse: the third string
    g = _seq_func(nn.Linear(64, 64), _MySoftplus() if name == "softplus" else _MyElu(), nn.Linear(64, 64))
    _, _, _, ode = _solve(g, pn_linear_bare=1, **{opt: "1"})
    assert status(ode) == "stock modules (no eligible Linear -> %s pair: a subclass of nn.Linear or nn.%s)" % (label, label)
    _, _, _, ode = _solve(g, **{opt: "1"})
    assert ode._fwd is None and status(ode).startswith("stock modules (no eligible pair")
    # -pn_linear_fwd 0 switches the pairs off with the others
    before = _n("fwd_" + name)
    _, _, _, ode = _solve(f, pn_linear_fwd=0, **{opt: "1"})
    assert ode._fwd is None and status(ode).startswith("stock modules") and _n("fwd_" + name) == before


def test_any_other_value_of_the_options_is_refused():
    f = _both_net()
    for opt in ("pn_linear_softplus", "pn_linear_elu"):
        for bad in ("2", "auto", "-1", "yes"):
            with pytest.raises(PnError, match="-%s must be 0 or 1" % opt):
                _solve(f, **{opt: bad})


def test_changing_an_option_between_two_solves_of_one_solver_reinstalls():
    f = _both_net()
    options.set_option("ts_adapt_type", "none")
    y0 = _y()
    ode = petsc_adjoint.ODEPetsc(backend=SoftplusEluOps)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    t = torch.tensor([0.0, 0.05], dtype=torch.float64)
    a = ode.odeint_adjoint(y0, t)
    assert ode.linear_elu == "off (-pn_linear_elu 0)" and NoGeluOps.calls == {}
    options.set_option("pn_linear_elu", "1")
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    b = ode.odeint_adjoint(y0, t)
    assert ode.linear_elu.startswith("fused (1 pairs") and ode.linear_softplus == "off (-pn_linear_softplus 0)"
    assert _n("fwd_elu") > 0 and _n("fwd_softplus") == 0 and rel_err(b, a) < 1e-6


# -------------------------------------------------------------------------------------------------------------------------- the C ABI
def _last_error(lib):
    return lib.pn_last_error().decode()


def test_the_c_entry_points_take_16_and_32_and_refuse_the_values_that_name_nothing():
    lib = _lib.load()
    assert _lib.PN_ACT_SOFTPLUS == 16 and _lib.PN_ACT_ELU == 32 and _lib.PN_ACT_GELU == 8 and _lib.PN_ACT_SIGMOID == 4
    assert _lib.PN_ABI_VERSION == 4 and lib.pn_abi_version() == 4
    n = 256 * 64
    big = torch.zeros(5 * n + 8)
    g, a, w, gz, dx = (big.data_ptr() + 4 * n * k for k in range(5))
    assert g % 16 == 0
    PLAIN = _lib.PN_LINEAR_FORM_PLAIN
    fwd_msg = ("pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU or PN_ACT_SOFTPLUS "
               "or PN_ACT_ELU")
    bwd_msg = ("pn_linear_bwd_act: act is PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU or PN_ACT_SOFTPLUS or PN_ACT_ELU "
               "(PN_ACT_IDENTITY: use pn_linear_dx)")
    p = big.data_ptr()
    for flags in (0, PLAIN):
        for act in (6, 9, 17, 33, 48, 3, 5, 7, -1):
            assert lib.pn_linear_bwd_act(None, 0, 256, 64, 64, g, a, w, act, gz, dx, flags) != 0 and _last_error(lib) == bwd_msg
            assert lib.pn_linear_fwd_form(None, 0, 256, 64, 64, p, p, None, act, p, flags) != 0 and _last_error(lib) == fwd_msg
            assert lib.pn_linear_fwd_pre(None, 0, 256, 64, 64, p, p, None, act, p, p + 4 * n, flags) != 0 and _last_error(lib) == fwd_msg
            assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, act, p) != 0 and _last_error(lib) == fwd_msg
        for act in (_lib.PN_ACT_SOFTPLUS, _lib.PN_ACT_ELU):
            # the new values reach the refusals behind the act's: shape, null, alignment, alias
            assert lib.pn_linear_bwd_act(None, 0, 128, 64, 64, g, a, w, act, gz, dx, flags) != 0
            assert "pn_linear_bwd: unsupported dtype or shape" in _last_error(lib)
            assert lib.pn_linear_bwd_act(None, 0, 256, 64, 64, g, None, w, act, gz, dx, flags) != 0 and "null operand" in _last_error(lib)
            assert lib.pn_linear_bwd_act(None, 0, 256, 64, 64, g, a + 4, w, act, gz, dx, flags) != 0 and "16-byte aligned" in _last_error(lib)
            for alias in (g, a, w, g + 16):
                assert lib.pn_linear_bwd_act(None, 0, 256, 64, 64, g, a, w, act, alias, dx, flags) != 0
                assert "gz must not alias g, a or w" in _last_error(lib)
            assert lib.pn_linear_bwd_act(None, 0, 256, 64, 64, g, a, w, act, gz, gz, flags) != 0
            assert "dx must not alias g, a, w or gz" in _last_error(lib)
            assert lib.pn_linear_fwd(None, 0, 256, 64, 64, p, p, None, act, p) != 0 and "y must not alias" in _last_error(lib)
            assert lib.pn_linear_fwd_form(None, 0, 256, 64, 64, p, p, None, act, p, flags) != 0 and "y must not alias" in _last_error(lib)
            assert lib.pn_linear_fwd_pre(None, 0, 256, 64, 64, p, p, None, act, p, p + 4 * n, flags) != 0 and "y must not alias" in _last_error(lib)
    assert not bool(big.any())
