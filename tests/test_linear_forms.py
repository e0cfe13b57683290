"""The form switch of pn_linear_fwd / pn_linear_bwd seen from the host: ``PN_LINEAR_FORM_PLAIN`` and ``-pn_linear_form auto|plain``.
No device is touched: the flag is checked in front of everything else, and the solves run on the CPU stand-in of test_linear_fwd.py,
which has no forms -- the option must leave it alone.  (That the two forms give the same bits: tests/test_gpu_linear_forms.py.)"""
import pytest
import torch

from pnode_amd import _lib, options, petsc_adjoint
from problems import MLPFunc, flat_grads
from test_linear_fwd import FwdOps


@pytest.fixture(autouse=True)
def _clean_options(monkeypatch):
    from pnode_amd import _linearfwd
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    options.clear()
    yield
    options.clear()


def test_the_option_takes_auto_and_plain_and_refuses_anything_else_by_name():
    assert options.linear_form() == "auto"
    for v in ("auto", "plain", "PLAIN"):
        options.set_option("pn_linear_form", v)
        assert options.linear_form() == v.lower()
    options.set_option("pn_linear_form", "wide")
    with pytest.raises(ValueError, match="pn_linear_form 'wide'"):
        options.linear_form()


def _last_error(lib):
    return lib.pn_last_error().decode()


def test_an_unknown_flag_is_refused_by_name_and_the_plain_flag_is_accepted():
    lib = _lib.load()
    assert _lib.PN_LINEAR_FORM_PLAIN == 1
    buf = torch.zeros(256 * 64)
    p = buf.data_ptr()
    for flags in (2, 4, 3, -2):
        assert lib.pn_linear_fwd_form(None, 0, 256, 64, 64, p, p, None, 1, p, flags) != 0
        assert "pn_linear_fwd_form: unknown flag" in _last_error(lib) and "PN_LINEAR_FORM_PLAIN" in _last_error(lib)
        assert lib.pn_linear_bwd_form(None, 0, 256, 64, 64, p, p, p, p, p, flags) != 0
        assert "pn_linear_bwd_form: unknown flag" in _last_error(lib)
    # 0 and PN_LINEAR_FORM_PLAIN get past the flag: what refuses these calls is the shape (rows < 256), in the words of the old entry points
    for flags in (0, _lib.PN_LINEAR_FORM_PLAIN):
        assert lib.pn_linear_fwd_form(None, 0, 128, 64, 64, p, p, None, 1, p, flags) != 0
        assert "pn_linear_fwd: unsupported dtype or shape" in _last_error(lib)
        assert lib.pn_linear_bwd_form(None, 0, 128, 64, 64, p, p, p, p, p, flags) != 0
        assert "pn_linear_bwd: unsupported dtype or shape" in _last_error(lib)
    assert lib.pn_linear_fwd(None, 0, 128, 64, 64, p, p, None, 1, p) != 0
    assert "pn_linear_fwd: unsupported dtype or shape" in _last_error(lib)
    assert not bool(buf.any())


def _solve(form):
    options.clear()
    options.set_option("ts_adapt_type", "none")
    if form is not None:
        options.set_option("pn_linear_form", form)
    FwdOps.fwd_calls = 0
    f = MLPFunc(64, std=0.1)
    y0 = torch.randn(256, 64, generator=torch.Generator().manual_seed(1))
    ode = petsc_adjoint.ODEPetsc(backend=FwdOps)
    ode.setupTS(y0, f, step_size=0.05, method="rk4")
    y = y0.clone().requires_grad_(True)
    out = ode.odeint_adjoint(y, torch.tensor([0.0, 0.15], dtype=torch.float64))
    out[-1].pow(2).sum().backward()
    return out.detach(), y.grad, flat_grads(f), ode


def test_the_host_stand_in_ignores_the_form():
    o0, y0, p0, ode0 = _solve(None)
    calls = FwdOps.fwd_calls
    assert calls > 0 and ode0._fwd is not None
    o1, y1, p1, ode1 = _solve("plain")
    assert FwdOps.fwd_calls == calls and ode1._fwd is not None and not hasattr(ode1._ops, "linear_flags")
    assert torch.equal(o0, o1) and torch.equal(y0, y1) and torch.equal(p0, p1)
    options.clear()
    options.set_option("pn_linear_form", "wide")
    with pytest.raises(ValueError, match="pn_linear_form"):
        _solve_keep = petsc_adjoint.ODEPetsc(backend=FwdOps)
        _solve_keep.setupTS(torch.zeros(256, 64), MLPFunc(64), step_size=0.05, method="rk4")
