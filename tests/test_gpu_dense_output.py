"""-pn_output_times interpolate on the MI355X: the two dense-output kernels (csrc/pn_dense.hip) against fp64 host sums, and the
C3b shape under every launch mode, step loop and trajectory mode (same bits), against the CPU stand-in on a shard."""
import math

import pytest
import torch

from conftest import require_gpu  # noqa: F401
from pnode_amd import _lib, options, petsc_adjoint
from pnode_amd._vecops import HipVecOps
from problems import MLPFunc, SwitchedMLPFunc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- kernels
def _ops(n, dtype):
    return HipVecOps(DEV, dtype, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [1, 3, 4097, 2 ** 21 + 5])
@pytest.mark.parametrize("m,nk", [(1, 1), (7, 4), (32, 6), (65, 7)])
@pytest.mark.parametrize("misaligned", [False, True])
def test_dense_kernels_against_fp64_sums(dtype, n, m, nk, misaligned):
    """Both kernels against fp64 sums in the SCALAR form: every n here is odd, so the row stride ld = n is no multiple of the
    vector width and the launchers' `vec` predicate is false with and without the one-element offset (asserted below).  The
    16-byte form is tested in test_gpu_kernel_variants.py."""
    g = torch.Generator(device="cpu").manual_seed(n * 7 + m)
    off = 1 if misaligned else 0
    ops = _ops(n, dtype)
    store = torch.randn(off + (nk + 1) * n, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    u = store[off: off + n]
    Ks = [store[off + (j + 1) * n: off + (j + 2) * n] for j in range(nk)]
    coefs = torch.randn(m, nk, generator=g, dtype=torch.float64) * 0.1
    out_store = torch.full((off + m * n,), float("nan"), dtype=dtype, device=DEV)
    out = out_store[off:].view(m, n)
    vw = 16 // store.element_size()
    assert out.stride(0) % vw != 0                     # dense_eval: vec = al16(...) && ld % VW == 0 is false
    ops.dense_eval(out, u, Ks, coefs.tolist())
    cq = coefs.to(dtype).double()                      # coefficients rounded once to the storage type
    ref = u.double().cpu()[None, :] + cq @ torch.stack([k.double().cpu() for k in Ks])
    tol = 1e-5 if dtype == torch.float32 else 1e-13
    assert float((out.double().cpu() - ref).abs().max()) <= tol * float(ref.abs().max())
    again = torch.empty_like(out)
    ops.dense_eval(again, u, Ks, coefs.tolist())
    assert torch.equal(again, out)

    # the transpose: D_j = sum_o c_oj g_o, G = sum_o g_o (+ accumulate)
    gst = torch.randn(off + m * n, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    gr = gst[off:].view(m, n)
    assert gr.stride(0) % vw != 0                      # dense_adjoint likewise
    dst = torch.full((off + (nk + 1) * n,), float("nan"), dtype=dtype, device=DEV)
    Ds = [dst[off + j * n: off + (j + 1) * n] for j in range(nk)]
    G = dst[off + nk * n: off + (nk + 1) * n]
    ops.dense_adjoint(Ds, G, gr, coefs.tolist())
    gd = gr.double().cpu()
    refD = cq.t() @ gd
    refG = gd.sum(0)
    tol = (1e-5 if dtype == torch.float32 else 1e-13) * math.sqrt(m)
    assert float((torch.stack([d.double().cpu() for d in Ds]) - refD).abs().max()) <= tol * max(float(refD.abs().max()), 1.0)
    assert float((G.double().cpu() - refG).abs().max()) <= tol * max(float(refG.abs().max()), 1.0)
    first = [d.clone() for d in Ds] + [G.clone()]
    ops.dense_adjoint(Ds, G, gr, coefs.tolist())
    assert all(torch.equal(a, b) for a, b in zip(first, Ds + [G]))
    ops.dense_adjoint(Ds, G, gr, coefs.tolist(), accumulate=True)
    assert float((torch.stack([d.double().cpu() for d in Ds]) - 2 * refD).abs().max()) <= 2 * tol * max(float(refD.abs().max()), 1.0)
    assert float((G.double().cpu() - 2 * refG).abs().max()) <= 2 * tol * max(float(refG.abs().max()), 1.0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- solves
def _solver(func, y0, method, opts, step=0.01, backend=None):
    options.clear()
    options.set_option("pn_output_times", "interpolate")
    for k, v in opts.items():
        options.set_option(k, v)
    ode = petsc_adjoint.ODEPetsc(backend=backend) if backend is not None else petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, func, step_size=step, method=method, enable_adjoint=True)
    options.clear()
    return ode


def _solve(ode, func, y0, t, w):
    for p in func.parameters():
        p.grad = None
    y = y0.detach().clone().requires_grad_(True)
    out = ode.odeint_adjoint(y, t)
    (out * w).sum().backward()
    return out.detach().clone(), y.grad.clone(), torch.cat([p.grad.reshape(-1) for p in func.parameters()])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _c3b(rows=4096):
    func = MLPFunc(d=512, dtype=torch.float32).to(DEV)
    y0 = (torch.randn(rows, 512, generator=torch.Generator().manual_seed(1)) * 0.5).to(DEV)
    return func, y0


def test_c3b_shape_modes_and_step_sequence():
    func, y0 = _c3b()
    t = torch.linspace(0, 1, 101, dtype=torch.float32, device=DEV)
    w = torch.randn((101, 4096, 512), generator=torch.Generator().manual_seed(2)).to(DEV) * 1e-3
    ends = _solver(func, y0, "dopri5", {"pn_graph_capture": "0"})
    _solve(ends, func, y0, t[[0, -1]], w[[0, -1]])
    base_ode = _solver(func, y0, "dopri5", {"pn_graph_capture": "0"})
    base = _solve(base_ode, func, y0, t, w)
    assert base_ode.step_log() == ends.step_log()
    assert base_ode.num_steps < 20
    for opts in ({"pn_graph_capture": "auto"}, {"pn_graph_capture": "1"}, {"pn_step_loop": "python", "pn_graph_capture": "0"}):
        ode = _solver(func, y0, "dopri5", opts)
        for call in range(4):                      # past the warm-up calls of the replaying modes
            got = _solve(ode, func, y0, t, w)
            assert ode.step_log() == ends.step_log(), (opts, call)
            assert _same(got, base), (opts, call, ode.graph_status)


def test_c3b_shard_matches_cpu_stand_in():
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _cpu_dense_ops import CpuDenseOps
    func, y0 = _c3b(64)
    t = torch.linspace(0, 1, 101, dtype=torch.float32)
    w = torch.randn((101, 64, 512), generator=torch.Generator().manual_seed(2)) * 1e-3
    gpu = _solve(_solver(func, y0, "dopri5", {}), func, y0, t.to(DEV), w.to(DEV))
    fc = MLPFunc(d=512, dtype=torch.float32)
    fc.load_state_dict({k: v.cpu() for k, v in func.state_dict().items()})
    cpu_ode = _solver(fc, y0.cpu(), "dopri5", {}, backend=CpuDenseOps)
    cpu = _solve(cpu_ode, fc, y0.cpu(), t, w)
    for a, b in zip(gpu, cpu):
        a = a.cpu()
        assert float((a - b).abs().max()) <= 2e-4 * float(b.abs().max()) + 1e-6


def test_rk4_off_grid_auto_gives_the_eager_bits():
    func, y0 = _c3b()
    t = torch.linspace(0, 1, 37, dtype=torch.float32, device=DEV)
    w = torch.randn((37, 4096, 512), generator=torch.Generator().manual_seed(4)).to(DEV) * 1e-3
    base = _solve(_solver(func, y0, "rk4", {"pn_graph_capture": "0", "ts_adapt_type": "none"}), func, y0, t, w)
    ode = _solver(func, y0, "rk4", {"pn_graph_capture": "auto", "ts_adapt_type": "none"})
    for call in range(4):
        assert _same(_solve(ode, func, y0, t, w), base), call
    st = ode.graph_status
    assert st.startswith("graph") or "-pn_output_times interpolate" in st, st


def test_switched_mlp_checkpoint_budget_same_bits():
    func = SwitchedMLPFunc(d=512, dtype=torch.float32).to(DEV)
    y0 = (torch.randn(256, 512, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV)
    t = torch.linspace(0, 1.0, 51, dtype=torch.float32, device=DEV)
    w = torch.randn((51, 256, 512), generator=torch.Generator().manual_seed(6)).to(DEV) * 1e-3
    runs = []
    for opts in ({"ts_trajectory_solution_only": "0"}, {"ts_trajectory_solution_only": "1"},
                 {"ts_trajectory_max_cps_ram": "3"}, {"ts_trajectory_max_cps_ram": "3", "ts_trajectory_solution_only": "0"}):
        ode = _solver(func, y0, "dopri5", dict(opts, pn_graph_capture="0"))
        runs.append((_solve(ode, func, y0, t, w), ode.step_log(), ode.num_rejections))
    assert len(runs[0][1]) > 3
    for r in runs[1:]:
        assert r[1] == runs[0][1]
        assert _same(r[0], runs[0][0])
