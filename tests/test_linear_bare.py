"""func's bare nn.Linear layers (pnode_amd/_linearfwd.py, ``-pn_linear_bare 0|1``): which layers are bare, that the default changes nothing,
what every other case falls back to, and the C entry points' refusals.  Host logic: ``pn_linear_fwd`` and ``pn_linear_dx`` are stood in
for by the torch expressions they replace (``F.linear``, ``matmul``), so every result must EQUAL the stock modules'."""
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _cpu_vecops import CpuVecOps
from pnode_amd import _funcguard, _lib, _linearfwd, options, petsc_adjoint
from problems import MLPFunc, flat_grads, rel_err


def _shapes(dtype, rows, out_f, in_f):
    return dtype == torch.float32 and rows >= 256 and out_f % 64 == 0 and in_f % 64 == 0


class NoDxOps(CpuVecOps):
    """The CPU stand-in with the entry points of pn_linear_fwd and pn_linear_bwd, none for pn_linear_dx."""
    fwd_calls = 0
    bare_fwd_calls = 0         # ... of them with the identity
    bwd_calls = 0

    def linear_fwd_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_fwd(self, x, w, b, tanh, y=None):
        assert self.linear_fwd_supported(x.shape[0], w.shape[0], w.shape[1]) and x.dim() == 2 and x.is_contiguous()
        NoDxOps.fwd_calls += 1
        NoDxOps.bare_fwd_calls += 0 if tanh else 1
        z = F.linear(x, w, b)
        return torch.tanh(z) if tanh else z

    def linear_bwd_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_bwd(self, g, a, w, gz=None, dx=None):
        NoDxOps.bwd_calls += 1
        gz = torch.ops.aten.tanh_backward(g, a)
        return gz, torch.matmul(gz, w)


class DxOps(NoDxOps):
    """... and with pn_linear_dx's: the same shapes, the library expression."""
    dx_calls = 0

    def linear_dx_supported(self, rows, out_f, in_f):
        return _shapes(self.dtype, rows, out_f, in_f)

    def linear_dx(self, g, w, dx=None):
        assert self.linear_dx_supported(g.shape[0], w.shape[0], w.shape[1]) and g.dim() == 2 and g.is_contiguous() and w.is_contiguous()
        DxOps.dx_calls += 1
        return torch.matmul(g, w)


class OffByAThousandthOps(DxOps):
    def linear_dx(self, g, w, dx=None):
        return super().linear_dx(g, w) * 1.001


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self, ops=DxOps):
        self._ops = ops(torch.device("cpu"), torch.float32, 256 * 64)


@pytest.fixture(autouse=True)
def _host_rules(monkeypatch):
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    NoDxOps.fwd_calls = NoDxOps.bare_fwd_calls = NoDxOps.bwd_calls = 0
    DxOps.dx_calls = 0
    options.clear()
    yield
    options.clear()


def _fwd(f, bare="1", bwd_mode="auto", ops=DxOps):
    ode = _Ode(ops)
    fwd = _linearfwd.LinearFwd(ode)
    fwd.keep = ode                                # (LinearFwd holds its solver weakly)
    if bare is None:
        on = fwd.install(f, list(f.parameters()), "auto", bwd_mode)
    else:
        on = fwd.install(f, list(f.parameters()), "auto", bwd_mode, bare)
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


def _eval(f, fwd, y, loss=lambda out: out.pow(2).sum()):
    with fwd.window():
        out = f(0.0, y)
    wrt = ([y] if y.requires_grad else []) + list(f.parameters())
    return out, torch.autograd.grad(loss(out), wrt)


def _stock(f, y, loss=lambda out: out.pow(2).sum()):
    out = f(0.0, y)
    return out, torch.autograd.grad(loss(out), ([y] if y.requires_grad else []) + list(f.parameters()))


# ---------------------------------------------------------------------------------------------------------------- plans and counts
def test_mlpfunc_with_the_option_on_runs_three_pairs_and_one_bare_layer_with_autograds_results():
    f = MLPFunc(64)
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, "1")
    assert on and fwd.active
    assert [(type(s), sorted(p)) for s, p in fwd.plans] == [(nn.Sequential, [0, 2, 4])]
    assert [(type(s), sorted(b)) for s, b in fwd.bare] == [(nn.Sequential, [6])]
    got, gg = _eval(f, fwd, y)
    assert NoDxOps.fwd_calls == 4 and NoDxOps.bare_fwd_calls == 1 and fwd.n_fused == 3 and fwd.n_bare == 1
    assert DxOps.dx_calls == 1 and fwd.n_bare_bwd == 1 and NoDxOps.bwd_calls == 3
    assert fwd.bare_checked and fwd.bare_bwd_checked and not fwd.bare_disabled and not fwd.bare_bwd_disabled
    assert fwd.bare_status == "fused (1 layers; 1 forward, 1 backward calls so far)"
    assert torch.equal(got, want)
    for a, b in zip(gg, gw):
        assert rel_err(a, b) < 1e-6
    assert "forward" not in f.net.__dict__
    f(0.0, y)
    assert NoDxOps.fwd_calls == 4


@pytest.mark.parametrize("bare", [None, "0"])
def test_by_default_and_with_0_nothing_changes(bare):
    f = MLPFunc(64)
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    fwd, _, on = _fwd(f, bare)
    assert on and [(type(s), sorted(p)) for s, p in fwd.plans] == [(nn.Sequential, [0, 2, 4])]
    got, gg = _eval(f, fwd, y)
    assert NoDxOps.fwd_calls == 3 and NoDxOps.bare_fwd_calls == 0 and DxOps.dx_calls == 0 and fwd.n_bare == 0 and fwd.n_bare_bwd == 0
    assert fwd.bare_status == "off (-pn_linear_bare 0)"
    assert torch.equal(got, want) and all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))


# ---------------------------------------------------------------------------------------------------------- other eligible shapes
def test_a_container_of_bare_layers_only_is_active_with_1_and_not_with_0():
    f = _seq_func(nn.Linear(64, 128), nn.ReLU(), nn.Linear(128, 64))
    fwd, _, on = _fwd(f, "0")
    assert not on and not fwd.active and fwd.plans == []
    fwd, _, on = _fwd(f, "1")
    assert on and fwd.active and fwd.plans == [] and [sorted(b) for _, b in fwd.bare] == [[0, 2]]
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    with fwd.window():
        assert "forward" in f.net.__dict__
    got, gg = _eval(f, fwd, y)
    assert NoDxOps.fwd_calls == 2 and NoDxOps.bare_fwd_calls == 2 and DxOps.dx_calls == 2 and fwd.n_bare == 2 and fwd.n_bare_bwd == 2
    assert torch.equal(got, want) and all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))
    assert "forward" not in f.net.__dict__


class _MyTanh(nn.Tanh):
    pass


class _MyLinear(nn.Linear):
    pass


def test_a_linear_in_front_of_a_tanh_subclass_is_a_bare_layer_followed_by_the_stock_module():
    f = _seq_func(nn.Linear(64, 64), _MyTanh(), nn.Linear(64, 64), nn.Tanh())
    fwd, _, on = _fwd(f, "1")
    assert on and [sorted(p) for _, p in fwd.plans] == [[2]] and [sorted(b) for _, b in fwd.bare] == [[0]]
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    got, gg = _eval(f, fwd, y)
    assert NoDxOps.fwd_calls == 2 and NoDxOps.bare_fwd_calls == 1 and DxOps.dx_calls == 1 and NoDxOps.bwd_calls == 1
    assert torch.equal(got, want) and all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))


# ------------------------------------------------------------------------------------------------- fallbacks to the stock module
def test_a_subclassed_linear_and_a_shared_weight_are_no_bare_layers():
    f = _seq_func(_MyLinear(64, 64), nn.ReLU(), nn.Linear(64, 64))
    fwd, _, on = _fwd(f, "1")
    assert on and [sorted(b) for _, b in fwd.bare] == [[2]]
    a, b = nn.Linear(64, 64), nn.Linear(64, 64)
    b.weight = a.weight
    f = _seq_func(a, nn.ReLU(), b)
    before = _funcguard.snapshot([f])
    fwd, _, on = _fwd(f, "1")
    assert not on and fwd.bare == [] and not fwd.active
    y = _y()
    with fwd.window():
        assert "forward" not in f.net.__dict__
        got = f(0.0, y)
    assert NoDxOps.fwd_calls == 0 and torch.equal(got, f(0.0, y)) and _funcguard.snapshot([f]) == before
    # a layer twice in the container, a frozen weight
    lin = nn.Linear(64, 64)
    assert _fwd(_seq_func(lin, nn.ReLU(), lin), "1")[0].bare == []
    f = _seq_func(nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64))
    f.net[0].weight.requires_grad_(False)
    assert [sorted(b) for _, b in _fwd(f, "1")[0].bare] == [[2]]


@pytest.mark.parametrize("where", ["layer", "container", "pre", "backward"])
def test_a_user_hook_on_the_layer_or_the_container_runs_the_stock_module(where):
    f = MLPFunc(64)
    fwd, _, _ = _fwd(f, "1")
    before = _funcguard.snapshot([f])
    seen = []
    if where == "pre":
        h = f.net[6].register_forward_pre_hook(lambda m, i: seen.append("pre"))
    elif where == "backward":
        h = f.net[6].register_full_backward_hook(lambda m, gi, go: None)
    else:
        m = {"layer": f.net[6], "container": f.net}[where]
        h = m.register_forward_hook(lambda m, i, o: seen.append(where))
    y = _y()
    with fwd.window():
        got = f(0.0, y)
    # a hook on the container: everything stock; on the bare layer: that layer only
    assert NoDxOps.bare_fwd_calls == 0 and NoDxOps.fwd_calls == (0 if where == "container" else 3) and "forward" not in f.net.__dict__
    assert torch.equal(got, f(0.0, y))
    if where != "backward":
        assert seen
    h.remove()
    assert _funcguard.snapshot([f]) == before
    NoDxOps.fwd_calls = 0
    with fwd.window():
        f(0.0, y)
    assert NoDxOps.fwd_calls == 4 and NoDxOps.bare_fwd_calls == 1


def test_a_global_hook_runs_the_stock_modules():
    f = MLPFunc(64)
    fwd, _, _ = _fwd(f, "1")
    h = torch.nn.modules.module.register_module_forward_hook(lambda m, i, o: None)
    try:
        with fwd.window():
            assert "forward" not in f.net.__dict__
            f(0.0, _y())
    finally:
        h.remove()
    assert NoDxOps.fwd_calls == 0


def test_under_autocast_and_for_a_non_contiguous_input_the_stock_module_runs():
    f = _seq_func(nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64))
    fwd, _, _ = _fwd(f, "1")
    y = _y()
    before = _funcguard.snapshot([f])
    with fwd.window():
        with torch.autocast("cpu", dtype=torch.bfloat16):
            f(0.0, y)
        assert NoDxOps.fwd_calls == 0
        f(0.0, _y(rows=255))                      # outside pn_linear_fwd_supported
        assert NoDxOps.fwd_calls == 0
        strided = _y(rows=512)[::2]
        got = f(0.0, strided)                     # not contiguous: the second layer only (its input is)
        assert NoDxOps.fwd_calls == 1 and torch.equal(got, f.net[2](torch.relu(f.net[0](strided))))
        f(0.0, y)
    assert NoDxOps.fwd_calls == 3 and NoDxOps.bare_fwd_calls == 3
    assert _funcguard.snapshot([f]) == before and "forward" not in f.net.__dict__


def test_func_is_left_as_found_when_an_evaluation_raises():
    class Boom(nn.Module):
        def forward(self, x):
            raise ValueError("boom")
    f = _seq_func(nn.Linear(64, 64), Boom())
    fwd, _, on = _fwd(f, "1")
    assert on
    before = _funcguard.snapshot([f])
    with pytest.raises(ValueError, match="boom"):
        with fwd.window():
            f(0.0, _y())
    assert NoDxOps.bare_fwd_calls == 1
    assert _funcguard.snapshot([f]) == before and "forward" not in f.net.__dict__


# ----------------------------------------------------------------------------------------------------------- backend and options
def test_option_bwd_0_and_a_backend_without_linear_dx_give_matmul_with_the_forward_still_fused():
    f = MLPFunc(64)
    y = _y().requires_grad_(True)
    want, gw = _stock(f, y)
    for kw in ({"bwd_mode": "0"}, {"ops": NoDxOps}):
        NoDxOps.fwd_calls = NoDxOps.bare_fwd_calls = 0
        fwd, _, _ = _fwd(f, "1", **kw)
        got, gg = _eval(f, fwd, y)
        assert NoDxOps.fwd_calls == 4 and NoDxOps.bare_fwd_calls == 1 and fwd.n_bare == 1
        assert DxOps.dx_calls == 0 and fwd.n_bare_bwd == 0
        assert torch.equal(got, want) and all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))
    # an input that needs no gradient: no dx at all
    one = _seq_func(nn.Linear(64, 64))
    fwd, _, _ = _fwd(one, "1")
    _, gg = _eval(one, fwd, _y())
    assert DxOps.dx_calls == 0 and fwd.n_bare == 1 and all(rel_err(a, b) < 1e-6 for a, b in zip(gg, _stock(one, _y())[1]))
    # a cotangent that is not contiguous (expanded by sum): matmul
    fwd, _, _ = _fwd(f, "1")
    got, gg = _eval(f, fwd, y, lambda out: out.sum())
    _, gw = _stock(f, y, lambda out: out.sum())
    assert DxOps.dx_calls == 0 and fwd.n_bare == 1 and all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))


def test_a_linear_dx_off_by_a_thousandth_switches_off_the_bare_backward_only():
    f = MLPFunc(64)
    y = _y().requires_grad_(True)
    _, gw = _stock(f, y)
    fwd, _, _ = _fwd(f, "1", ops=OffByAThousandthOps)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, g1 = _eval(f, fwd, y)
        _, g2 = _eval(f, fwd, y)
    msgs = [str(c.message) for c in caught if "bare Linear layers runs matmul" in str(c.message)]
    assert len(msgs) == 1 and "dx by" in msgs[0]
    assert DxOps.dx_calls == 1 and fwd.n_bare_bwd == 0 and fwd.bare_bwd_disabled and "pn_linear_dx and matmul differ" in fwd.bare_bwd_why
    # the bare forward and the pairs, forward and backward, stay fused
    assert not fwd.bare_disabled and fwd.n_bare == 2 and not fwd.disabled and fwd.n_fused == 6
    assert not fwd.bwd_disabled and fwd.n_fused_bwd == 6 and NoDxOps.bwd_calls == 6
    for gg in (g1, g2):
        assert all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))


def test_a_failed_bare_forward_check_switches_off_the_bare_path_only(monkeypatch):
    f = MLPFunc(64)
    fwd, ode, _ = _fwd(f, "1")
    good = ode._ops.linear_fwd
    monkeypatch.setattr(ode._ops, "linear_fwd", lambda x, w, b, tanh, y=None: good(x, w, b, tanh) + (0.0 if tanh else 1e-3))
    y = _y()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with fwd.window():
            got = f(0.0, y)
    assert fwd.bare_disabled and "differ by" in fwd.bare_why and [c for c in caught if "bare Linear layers" in str(c.message)]
    assert fwd.bare_status.startswith("stock modules (pn_linear_fwd and F.linear differ")
    assert not fwd.disabled and fwd.n_fused == 3 and fwd.active and fwd.n_bare == 0
    assert torch.equal(got, f(0.0, y))
    with fwd.window():
        f(0.0, y)
    assert fwd.n_fused == 6 and fwd.n_bare == 0


# -------------------------------------------------------------------------------------------------------------- solves and the ABI
def _solve(f, bare, backend=DxOps, steps=3):
    options.clear()
    options.set_option("ts_adapt_type", "none")
    if bare is not None:
        options.set_option("pn_linear_bare", bare)
    y0 = _y()
    ode = petsc_adjoint.ODEPetsc(backend=backend)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    for p in f.parameters():
        p.grad = None
    y = y0.clone().requires_grad_(True)
    out = ode.odeint_adjoint(y, torch.tensor([0.0, 0.05 * steps], dtype=torch.float64))
    out[-1].pow(2).sum().backward()
    return out.detach().clone(), y.grad.clone(), flat_grads(f).clone(), ode


def test_a_whole_solve_with_the_option_on_gives_the_solution_bits_and_gradients_of_0():
    f = MLPFunc(64, std=0.1)
    o0, y0, p0, ode0 = _solve(f, "0")
    assert DxOps.dx_calls == 0 and NoDxOps.bare_fwd_calls == 0 and ode0.linear_bare == "off (-pn_linear_bare 0)"
    assert ode0._fwd.n_fused > 0 and ode0._fwd.n_bare == 0
    on, yn, pn, oden = _solve(f, None)
    assert DxOps.dx_calls == 0 and NoDxOps.bare_fwd_calls == 0 and oden.linear_bare == "off (-pn_linear_bare 0)"
    assert torch.equal(on, o0) and torch.equal(yn, y0) and torch.equal(pn, p0)
    o1, y1, p1, ode1 = _solve(f, "1")
    fwd = ode1._fwd
    # rk4 x 3 steps: at least four stage evaluations and four stage VJPs per step, one bare layer each
    assert fwd.n_bare >= 3 * 4 * 2 and NoDxOps.bare_fwd_calls == fwd.n_bare and 3 * fwd.n_bare == fwd.n_fused
    assert fwd.n_bare_bwd >= 3 * 4 and DxOps.dx_calls == fwd.n_bare_bwd and 3 * fwd.n_bare_bwd == fwd.n_fused_bwd
    assert ode1.linear_bare == "fused (1 layers; %d forward, %d backward calls so far)" % (fwd.n_bare, fwd.n_bare_bwd)
    assert ode1.linear_fwd.startswith("fused (3 pairs") and ode1.linear_bwd.startswith("fused (")
    assert ode1.linear_param_grads.startswith("engine") and ode1._lin.n_autograd == 0 and ode1._lin.n_clean > 0
    assert torch.equal(o1, o0) and rel_err(y1, y0) < 1e-6 and rel_err(p1, p0) < 1e-6


def test_a_solve_over_a_container_of_bare_layers_only():
    f0 = _seq_func(nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64))
    o0, y0, p0, ode0 = _solve(f0, "0")
    assert ode0._fwd is None and ode0.linear_bare == "off (-pn_linear_bare 0)" and NoDxOps.fwd_calls == 0
    o1, y1, p1, ode1 = _solve(f0, "1")
    assert ode1._fwd is not None and ode1._fwd.n_bare > 0 and ode1._fwd.n_bare_bwd > 0 and ode1.linear_bare.startswith("fused (2 layers")
    assert ode1.linear_fwd.startswith("stock modules") and ode1._lin.n_autograd == 0
    assert torch.equal(o1, o0) and rel_err(y1, y0) < 1e-6 and rel_err(p1, p0) < 1e-6
    # -pn_linear_fwd 0 switches the bare layers off with the pairs
    options.clear()
    options.set_option("pn_linear_fwd", "0")
    options.set_option("pn_linear_bare", "1")
    ode = petsc_adjoint.ODEPetsc(backend=DxOps)
    ode.setupTS(_y(), f0, step_size=0.05, method="rk4")
    assert ode._fwd is None and ode.linear_bare.startswith("stock modules")


def _last_error(lib):
    return lib.pn_last_error().decode()


def test_pn_linear_dx_form_refuses_an_unknown_flag_and_an_unsupported_shape_by_name():
    lib = _lib.load()
    buf = torch.zeros(256 * 64)
    p = buf.data_ptr()
    for flags in (2, 4, 3, -2):
        assert lib.pn_linear_dx_form(None, 0, 256, 64, 64, p, p, p, flags) != 0
        assert "pn_linear_dx_form: unknown flag" in _last_error(lib) and "PN_LINEAR_FORM_PLAIN" in _last_error(lib)
        # (the flag is checked first: the shape of this call is refused too)
        assert lib.pn_linear_dx_form(None, 0, 128, 64, 64, p, p, p, flags) != 0
        assert "pn_linear_dx_form: unknown flag" in _last_error(lib)
    for flags in (0, _lib.PN_LINEAR_FORM_PLAIN):
        assert lib.pn_linear_dx_form(None, 0, 128, 64, 64, p, p, p, flags) != 0
        assert "pn_linear_dx: unsupported dtype or shape" in _last_error(lib)
        assert lib.pn_linear_dx_form(None, 1, 256, 64, 64, p, p, p, flags) != 0                    # fp64
        assert "pn_linear_dx: unsupported dtype or shape" in _last_error(lib)
    assert lib.pn_linear_dx(None, 0, 128, 64, 64, p, p, p) != 0
    assert "pn_linear_dx: unsupported dtype or shape" in _last_error(lib)
    # a null operand, an operand off 16 bytes, dx sharing a byte with g or w: refused in this order, nothing launched
    big = torch.zeros(3 * 256 * 64 + 8)
    g, w, dx = big.data_ptr(), big.data_ptr() + 4 * 256 * 64, big.data_ptr() + 8 * 256 * 64
    assert g % 16 == 0
    for args in ((None, w, dx), (g, None, dx), (g, w, None)):
        assert lib.pn_linear_dx(None, 0, 256, 64, 64, *args) != 0 and "pn_linear_dx: null operand" in _last_error(lib)
    for args in ((g + 4, w, dx), (g, w + 8, dx), (g, w, dx + 4)):
        assert lib.pn_linear_dx(None, 0, 256, 64, 64, *args) != 0 and "16-byte aligned" in _last_error(lib)
    for args in ((g, w, g), (g, w, g + 16), (g, w, w), (g, w, w + 4 * 64 * 64 - 16), (g, dx, dx)):
        assert lib.pn_linear_dx(None, 0, 256, 64, 64, *args) != 0 and "dx must not alias g or w" in _last_error(lib)
    assert not bool(buf.any()) and not bool(big.any())


def test_pn_linear_dx_supported_is_pn_linear_bwd_supported_on_a_grid_of_shapes():
    lib = _lib.load()
    n = yes = 0
    for dtype in (0, 1, 2):
        for rows in (0, 128, 255, 256, 257, 320, 4096, (1 << 30) - 1, 1 << 30):
            for out_f in (0, 32, 48, 64, 96, 100, 128, 512, 1 << 30):
                for in_f in (0, 32, 64, 96, 128, 192, 500, 512, 1 << 30):
                    got = lib.pn_linear_dx_supported(dtype, rows, out_f, in_f)
                    assert got == lib.pn_linear_bwd_supported(dtype, rows, out_f, in_f), (dtype, rows, out_f, in_f)
                    n += 1
                    yes += got
    assert 0 < yes < n
