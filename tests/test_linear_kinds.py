"""The table of kinds of owned layer (pnode_amd/_linearfwd.py, ``KINDS``): that it names the seven kinds and every ``LinearFwd`` has one
record per row, that every name ``LinearFwd`` has had for a field of a record still reads that field, and that one window over a net
with all seven kinds in it runs each of them once, forward and backward, through the entry its row names.  Host logic: the kernels are
stood in for by their formulas spelled in torch (tests/_cpu_linear_softplus_elu.py), so outputs and gradients agree with the stock
modules' to 1e-6 in the relative 2-norm, the bar of tests/test_linear_softplus_elu.py for the same stand-ins."""
import warnings

import pytest
import torch
import torch.nn as nn

from _cpu_linear_gelu import NoGeluOps
from _cpu_linear_softplus_elu import SoftplusEluOps
from pnode_amd import _linearfwd
from problems import rel_err

KEYS = ["tanh", "relu", "sigmoid", "gelu", "softplus", "elu", "bare"]
ACTS = [nn.Tanh, nn.ReLU, nn.Sigmoid, nn.GELU, nn.Softplus, nn.ELU]

# the names tests, tools and the solver read on a LinearFwd, by the kind whose record holds the value
NAMES = {
    "tanh": "plans mode disabled why checked n_fused bwd_mode bwd_disabled bwd_why bwd_checked n_fused_bwd",
    "bare": "bare bare_mode bare_disabled bare_why bare_checked n_bare bare_bwd_disabled bare_bwd_why bare_bwd_checked n_bare_bwd "
            "bare_active bare_status",
    "relu": "relu relu_mode relu_disabled relu_why relu_checked n_relu relu_bwd_disabled relu_bwd_why relu_bwd_checked n_relu_bwd "
            "relu_active relu_status",
    "sigmoid": "sig sigmoid sigmoid_active sigmoid_status n_sigmoid n_sigmoid_bwd",
    "gelu": "gelu gelu_active gelu_status n_gelu n_gelu_bwd",
    "softplus": "softplus softplus_status",
    "elu": "elu elu_status",
}


class _Ode(object):
    tensor_dtype = torch.float32
    _lin = None

    def __init__(self):
        self._ops = SoftplusEluOps(torch.device("cpu"), torch.float32, 256 * 64)


@pytest.fixture(autouse=True)
def _host_rules(monkeypatch):
    monkeypatch.setattr(_linearfwd.LinearFwd, "device_type", "cpu")
    NoGeluOps.calls = {}


class _Func(nn.Module):
    """A Linear in front of each of the six activations, and a closing bare Linear."""
    def __init__(self, d=64):
        super().__init__()
        torch.manual_seed(7)
        layers = []
        for cls in ACTS:
            layers += [nn.Linear(d, d), cls()]
        self.net = nn.Sequential(*(layers + [nn.Linear(d, d)]))

    def forward(self, t, y):
        return self.net(y)


def _installed(f):
    ode = _Ode()
    fwd = _linearfwd.LinearFwd(ode)
    fwd.keep = ode                                # (LinearFwd holds its solver weakly)
    assert fwd.install(f, list(f.parameters()), "1", "1", "1", "1", "1", "1", "1", "1")
    return fwd


def _run(f, fwd, y):
    with fwd.window():
        out = f(0.0, y)
    return out, torch.autograd.grad(out.pow(2).sum(), [y] + list(f.parameters()))


def test_the_table_names_the_seven_kinds_and_a_solver_has_a_record_of_each():
    assert [k.key for k in _linearfwd.KINDS] == KEYS
    assert [k.module for k in _linearfwd.PAIRS] == ACTS and _linearfwd.BARE is _linearfwd.KINDS[-1]
    fwd = _linearfwd.LinearFwd(_Ode())
    assert list(fwd.records) == KEYS and all(fwd.records[k.key].kind is k for k in _linearfwd.KINDS)
    assert len({id(st) for st in fwd.records.values()}) == 7
    assert fwd.kinds == (fwd.records["softplus"], fwd.records["elu"])
    for cls, key in zip(ACTS, KEYS):
        assert fwd._state(cls()) is fwd.records[key]
    assert fwd._state(nn.Linear(2, 2)) is None and fwd._state(nn.SiLU()) is None


@pytest.mark.parametrize("kind", _linearfwd.KINDS, ids=KEYS)
def test_every_legacy_name_reads_its_field_of_the_record(kind):
    f = _Func()
    fwd = _installed(f)
    y = torch.randn(256, 64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    st = fwd.records[kind.key]
    assert set(NAMES[kind.key].split()) <= set(kind.legacy)
    for when in ("installed", "run"):
        for name, field in kind.legacy.items():
            got, want = getattr(fwd, name), st if field is None else getattr(st, field)
            assert got is want or got == want, (when, name, field)
            with pytest.raises(AttributeError):
                setattr(fwd, name, got)           # read-only: the record is the storage
        if when == "installed":
            _run(f, fwd, y)
    assert (st.n, st.n_bwd, st.checked, st.bwd_checked, st.mode) == (1, 1, True, True, "1")
    assert fwd.bwd_mode == "1" and fwd.active and st.active and st.status.startswith("fused (1 ")


def test_one_window_runs_every_kind_once_forward_and_backward():
    f = _Func()
    y = torch.randn(256, 64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    want = f(0.0, y)
    gw = torch.autograd.grad(want.pow(2).sum(), [y] + list(f.parameters()))
    fwd = _installed(f)
    assert [sorted(p) for _, p in fwd.bare] == [[12]]
    for i, key in enumerate(KEYS[:-1]):
        assert [(type(s), sorted(p)) for s, p in fwd.records[key].plans] == [(nn.Sequential, [2 * i])]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got, gg = _run(f, fwd, y)
    for key in KEYS:
        st = fwd.records[key]
        assert (st.n, st.n_bwd) == (1, 1) and not st.disabled and not st.bwd_disabled and st.refused is None, key
        assert st.n_pre == (1 if key == "gelu" else 0)
    log = {"fwd_gelu_pre": 1, "fwd_identity": 1, "dx": 1}
    log.update({"fwd_" + key: 1 for key in KEYS[:-1] if key != "gelu"})
    log.update({"bwd_" + key: 1 for key in KEYS[:-1]})
    assert NoGeluOps.calls == log
    assert "forward" not in f.net.__dict__
    assert rel_err(got, want) < 1e-6 and all(rel_err(a, b) < 1e-6 for a, b in zip(gg, gw))
