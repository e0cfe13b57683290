"""RKSweep._vjp_results, the one clean-up of autograd's results behind every stage VJP (the batch sweep's _vjp, the per-sample
sweep, _add_param_grads(cotangent=...)), on the cases its docstring names.  Through the whole batch solver the aliasing cases are
pinned by test_host_engine.py::test_parameter_gradient_that_aliases_the_cotangent_buffer and
::test_parameter_gradient_that_is_a_small_view_of_the_cotangent_buffer; here the helper itself, so that the callers that do not go
through _vjp stand on the same ground."""
import torch

from _cpu_vecops import CpuVecOps
from problems import SpiralFunc
from pnode_amd import options, petsc_adjoint


def _solver():
    options.clear()
    ode = petsc_adjoint.ODEPetsc(backend=CpuVecOps)
    ode.setupTS(torch.zeros(4, 2, dtype=torch.float64), SpiralFunc(torch.float64), step_size=0.05, method="rk4")
    assert ode.tensor_dtype == torch.float64
    return ode


def _shares(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def test_what_shares_the_cotangents_storage_is_copied_whatever_its_size():
    ode = _solver()
    w = torch.arange(8, dtype=torch.float64)
    own = torch.full((3,), 2.0, dtype=torch.float64)
    grads = (w, w[:2], w.view(4, 2)[1], w[5], own, None)          # the cotangent itself, views of other sizes, a 0-dim select
    gy, gp = ode._vjp_results(None, grads, w)
    assert gy is None and len(gp) == len(grads) and gp[5] is None
    for got, g in zip(gp[:4], grads[:4]):
        assert not _shares(got, w) and got.is_contiguous() and got.shape == g.shape and torch.equal(got, g)
    assert gp[4] is own                                           # a gradient with storage of its own is handed through
    before = [g.clone() for g in gp[:5]]
    w.fill_(-1.0)                                                 # the sweep rewrites its cotangent buffer in place ...
    assert all(torch.equal(a, b) for a, b in zip(gp[:5], before))  # ... and what was queued still holds the gradients


def test_immediate_accumulation_copies_nothing():
    ode = _solver()
    w = torch.arange(8, dtype=torch.float64)
    gy, gp = ode._vjp_results(w.view(4, 2), (w, w[:2], None), w, deferred=False)
    assert gp[0] is w and _shares(gp[1], w) and gp[2] is None
    assert gy.shape == (8,) and _shares(gy, w)                    # (the callers copy a state cotangent that IS their buffer)


def test_dtype_and_layout():
    ode = _solver()
    w = torch.arange(8, dtype=torch.float64)
    g32 = torch.tensor([1.5, -2.25, 3.0], dtype=torch.float32)
    strided = torch.arange(12, dtype=torch.float64).view(3, 4).t()
    gy, gp = ode._vjp_results(torch.arange(8, dtype=torch.float32).view(2, 4).t(), (g32, strided), w)
    assert gy.dtype == torch.float64 and gy.shape == (8,) and gy.is_contiguous()
    assert torch.equal(gy, torch.tensor([0, 4, 1, 5, 2, 6, 3, 7], dtype=torch.float64))
    assert gp[0].dtype == torch.float64 and torch.equal(gp[0], g32.double())
    assert gp[1].is_contiguous() and gp[1].shape == (4, 3) and torch.equal(gp[1], strided)
