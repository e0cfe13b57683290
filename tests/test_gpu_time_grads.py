"""dL/dt on the MI355X: the two reductions of csrc/pn_tgrad.hip against fp64 host sums (bit-reproducible), the end-to-end time
gradient against the CPU stand-in, fp32 at C3a width against the fp64 engine, and the declined capture."""
import pytest
import torch
import torch.nn as nn

from conftest import require_gpu  # noqa: F401
from _cpu_tgrad_ops import CpuTgradOps
from pnode_amd import options, petsc_adjoint
from pnode_amd._vecops import HipVecOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class TMLP(nn.Module):
    def __init__(self, d, dtype, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.lin = nn.Linear(d, d)
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5)
            self.lin.bias.copy_(0.1 * torch.randn(d, generator=g, dtype=torch.float64))
        self.to(dtype)

    def forward(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        return torch.tanh(self.lin(y)) * (1.0 + 0.5 * torch.sin(3.0 * t)) + 0.2 * torch.cos(2.0 * t)


def _rows(count, n, dtype, misaligned, g):
    """`count` vectors of n elements in one allocation, row stride ld.  Aligned: every row starts on a 16-byte boundary and ld
    is a multiple of the vector width (the kernels' 16-byte form runs, with its ragged tail when n % VW != 0).  Misaligned: the
    same stride behind one element of offset, so no row is 16-byte aligned (the scalar form runs)."""
    vw = 16 // torch.empty((), dtype=dtype).element_size()
    ld = -(-n // vw) * vw
    off = 1 if misaligned else 0
    st = torch.randn(off + count * ld, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    rows = st[off:].view(count, ld)[:, :n]
    if not misaligned:
        assert all(r.data_ptr() % 16 == 0 for r in rows) and rows.stride(0) % vw == 0
    else:
        assert all(r.data_ptr() % 16 != 0 for r in rows)
    return rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [1, 5, 4097, 4099, 2 ** 20 + 3])
@pytest.mark.parametrize("misaligned", [False, True])
def test_tgrad_kernels_against_fp64_sums(dtype, n, misaligned):
    """Both reductions on ragged n (n % VW != 0: the vector form's tail), on the 16-byte form and on the scalar form."""
    g = torch.Generator().manual_seed(n)
    ops = HipVecOps(DEV, dtype, n)
    for np_ in (1, 3, 7):
        rows = _rows(2 * np_, n, dtype, misaligned, g)
        xs = [rows[p] for p in range(np_)]
        ys = [rows[np_ + p] for p in range(np_)]
        cs = torch.randn(np_, generator=g, dtype=torch.float64).tolist()
        acc = torch.full((3,), 0.5, dtype=torch.float64, device=DEV)
        ops.tgrad_dots(acc[1:2], xs, ys, cs, accumulate=True)
        ref = 0.5 + sum(c * float(x.double().cpu() @ y.double().cpu()) for c, x, y in zip(cs, xs, ys))
        assert abs(float(acc[1]) - ref) <= 1e-12 * max(1.0, abs(ref)) * (n ** 0.5)
        assert float(acc[0]) == 0.5 and float(acc[2]) == 0.5
        again = acc.clone()
        ops.tgrad_dots(again[1:2], xs, ys, cs, accumulate=False)
        ops.tgrad_dots(again[1:2], xs, ys, cs, accumulate=True)
        first = acc.clone()
        ops.tgrad_dots(first[1:2], xs, ys, cs, accumulate=False)
        ops.tgrad_dots(first[1:2], xs, ys, cs, accumulate=True)
        assert torch.equal(first, again)                         # bitwise over two runs
    for m, nk in ((1, 1), (5, 4), (32, 7), (33, 6)):
        gr = _rows(m, n, dtype, misaligned, g)
        kr = _rows(nk, n, dtype, misaligned, g)
        Ks = [kr[j] for j in range(nk)]
        co = torch.randn(m, nk, generator=g, dtype=torch.float64)
        acc = torch.zeros(m + 2, dtype=torch.float64, device=DEV)
        ops.dense_tgrad(acc[1:m + 1], gr, Ks, co.tolist(), accumulate=False)
        ref = ((gr.double().cpu() @ torch.stack([k.double().cpu() for k in Ks]).t()) * co).sum(1)
        a = acc.cpu()
        assert float(a[0]) == 0.0 and float(a[m + 1]) == 0.0
        assert float((a[1:m + 1] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())) * (n ** 0.5)
        b = acc.clone()
        ops.dense_tgrad(b[1:m + 1], gr, Ks, co.tolist(), accumulate=True)
        c = acc.clone()
        ops.dense_tgrad(c[1:m + 1], gr, Ks, co.tolist(), accumulate=True)
        assert torch.equal(b, c) and torch.allclose(b[1:m + 1], 2 * acc[1:m + 1], rtol=1e-14, atol=0)


def _solve(func, y0, t, method, mode, device, backend=None, extra=()):
    options.clear()
    options.set_option("pn_output_times", mode)
    options.set_option("pn_graph_capture", "0")
    for k, v in extra:
        options.set_option(k, v)
    ode = petsc_adjoint.ODEPetsc(backend=backend)
    ode.setupTS(y0.to(device), func, step_size=0.05, method=method)
    yy = y0.to(device).clone().requires_grad_(True)
    tt = t.to(device).clone().requires_grad_(True)
    y = ode.odeint_adjoint(yy, tt)
    w = torch.linspace(0.5, 1.5, y[0].numel(), dtype=y.dtype, device=device).view_as(y[0])
    sum((y[i] * w * (1 + 0.1 * i)).sum() for i in range(y.shape[0])).backward()
    options.clear()
    return tt.grad.detach().cpu().double(), ode


@pytest.mark.parametrize("method,mode", [("rk4", "match"), ("dopri5", "match"), ("dopri5", "interpolate"), ("bosh3", "interpolate")])
def test_end_to_end_fp64_against_cpu(method, mode):
    torch.manual_seed(0)
    y0 = torch.randn(64, 16, dtype=torch.float64)
    t = torch.tensor([0.1, 0.33, 0.5, 0.77, 0.9], dtype=torch.float64)
    fc = TMLP(16, torch.float64)
    fg = TMLP(16, torch.float64).to(DEV)
    ref, _ = _solve(fc, y0, t, method, mode, torch.device("cpu"), CpuTgradOps)
    got, _ = _solve(fg, y0, t, method, mode, DEV)
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    again, _ = _solve(fg, y0, t, method, mode, DEV)
    assert torch.equal(got, again)


def test_fp32_at_c3a_width_against_fp64():
    torch.manual_seed(0)
    y0 = torch.randn(4096, 512, dtype=torch.float64) * 0.5
    t = torch.tensor([0.0, 0.3, 0.5], dtype=torch.float64)
    f64 = TMLP(512, torch.float64).to(DEV)
    f32 = TMLP(512, torch.float32).to(DEV)
    ref, _ = _solve(f64, y0, t, "rk4", "match", DEV, extra=(("ts_adapt_type", "none"),))
    got, _ = _solve(f32, y0.float(), t.float(), "rk4", "match", DEV, extra=(("ts_adapt_type", "none"),))
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_capture_is_declined_while_t_requires_grad():
    options.clear()
    options.set_option("ts_adapt_type", "none")
    options.set_option("pn_graph_capture", "1")
    f = TMLP(8, torch.float32).to(DEV)
    y0 = torch.randn(16, 8, device=DEV)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, f, step_size=0.1, method="rk4")
    t = torch.tensor([0.0, 0.5], device=DEV)
    for _ in range(4):
        tt = t.clone().requires_grad_(True)
        ode.odeint_adjoint(y0.clone().requires_grad_(True), tt).sum().backward()
        assert tt.grad is not None
    assert ode.graph_status.startswith("eager (t requires grad")
    options.clear()
