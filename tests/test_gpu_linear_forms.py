"""-m gpu: the two forms of the K loop of pn_linear_fwd / pn_linear_bwd (csrc/pn_linear.hip) give the same bits.

The pipelined form (what aligned shapes take by themselves) keeps three LDS buffers, two sets of fragment registers and two sets of load
registers in rotation; the plain form (PN_LINEAR_FORM_PLAIN) is the loop the ragged bodies run.  Every accumulator takes the same MFMAs in
the same order in both, so y, gz and dx must be torch.equal.  K (in_f forward, out_f backward) over 64 .. 320 is 2, 4, 6, 8, 10 slabs:
fewer slabs than buffers, and every residue of the slab count modulo 3 and modulo 2 -- where a prologue, a drain or a rotation goes wrong.
Operands: random normal, and `distinct`: a different value in every (row, k) position, small integers times powers of two whose products
and sums stay exact in fp32 -- a fragment taken from the wrong slab, buffer or register set changes such a result outright, not its rounding.
rows 256 / 384 and 128 / 256 output columns: 4 to 12 workgroups, both tile columns of a workgroup row."""
import pytest
import torch
import torch.nn.functional as F

from _linear_tile_cases import distinct as _distinct
from conftest import require_gpu

pytestmark = pytest.mark.gpu

ROWS = [256, 384]
WIDTHS = [128, 256]                   # the output's columns: out_f forward, in_f backward
KS = [64, 128, 192, 256, 320]         # the product's K: in_f forward, out_f backward
PLAIN = 1                             # PN_LINEAR_FORM_PLAIN


def _ops(n):
    from pnode_amd import _lib
    from pnode_amd._vecops import HipVecOps
    assert _lib.PN_LINEAR_FORM_PLAIN == PLAIN
    return HipVecOps(require_gpu(), torch.float32, n)


def _operands(kind, rows, k, width, seed, dev):
    """A rows x k, B width x k (forward's layout), bias width."""
    if kind == "normal":
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(rows, k, generator=g).to(dev), (torch.randn(width, k, generator=g) / k ** 0.5).to(dev),
                torch.randn(width, generator=g).to(dev))
    return _distinct(rows, k, seed).to(dev), _distinct(width, k, seed + 17).to(dev), _distinct(1, width, seed + 5).view(-1).to(dev)


@pytest.mark.parametrize("kind", ["normal", "distinct"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("out_f", WIDTHS)
def test_forward_forms_give_the_same_bits(kind, rows, out_f):
    ops = _ops(rows * max(KS))
    for in_f in KS:
        x, w, b = _operands(kind, rows, in_f, out_f, rows + out_f + in_f, ops.device)
        for bias in (True, False):
            for tanh in (False, True):
                bb = b if bias else None
                plain = ops.linear_fwd(x, w, bb, tanh, flags=PLAIN)
                auto = ops.linear_fwd(x, w, bb, tanh)
                assert torch.equal(auto, plain), (in_f, bias, tanh, float((auto - plain).abs().max()))
        if kind == "distinct":
            # the operands are what they claim: the plain form gives the exact product
            z64 = F.linear(x.double(), w.double(), b.double())
            assert torch.equal(ops.linear_fwd(x, w, b, False, flags=PLAIN), z64.float())


@pytest.mark.parametrize("kind", ["normal", "distinct"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("in_f", WIDTHS)
def test_backward_forms_give_the_same_bits(kind, rows, in_f):
    ops = _ops(rows * max(KS))
    for out_f in KS:
        g, wt, _ = _operands(kind, rows, out_f, in_f, 2 * rows + in_f + out_f, ops.device)
        w = wt.t().contiguous()                   # out_f x in_f
        if kind == "normal":
            a = torch.tanh(torch.randn(rows, out_f, generator=torch.Generator().manual_seed(out_f)).to(ops.device))
        else:
            # 1 - a^2 in {1, 0}: gz is g with every third position struck out
            a = ((torch.arange(rows).view(-1, 1) + torch.arange(out_f).view(1, -1)) % 3 == 0).float().to(ops.device)
        gz0, dx0 = ops.linear_bwd(g, a, w, flags=PLAIN)
        gz1, dx1 = ops.linear_bwd(g, a, w)
        assert torch.equal(gz1, gz0), (out_f, float((gz1 - gz0).abs().max()))
        assert torch.equal(dx1, dx0), (out_f, float((dx1 - dx0).abs().max()))
        if kind == "distinct":
            gz64 = g.double() * (1.0 - a.double() ** 2)
            assert torch.equal(gz0, gz64.float()) and torch.equal(dx0, (gz64 @ w.double()).float())


def test_a_ragged_shape_still_runs_the_plain_body_and_meets_the_librarys_bars():
    """rows = 320: the ragged instantiations, whatever the flag; the bars of test_gpu_linear_fwd.py (2 x the library path's own error
    from float64) and of test_gpu_linear_bwd.py (1.5 x)."""
    rows, out_f, in_f = 320, 128, 192
    ops = _ops(rows * in_f)
    x, w, b = _operands("normal", rows, in_f, out_f, 9, ops.device)
    y = ops.linear_fwd(x, w, b, True)
    assert torch.equal(y, ops.linear_fwd(x, w, b, True, flags=PLAIN))
    z64 = F.linear(x.double(), w.double(), b.double())
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    e_lib = float(((torch.tanh(F.linear(x, w, b)).double() - torch.tanh(z64)).abs() / scale).max())
    e_own = float(((y.double() - torch.tanh(z64)).abs() / scale).max())
    print("ragged fwd: pn_linear_fwd %.3e  library %.3e" % (e_own, e_lib))
    assert e_own <= 2.0 * e_lib
    g = torch.randn(rows, out_f, generator=torch.Generator().manual_seed(4)).to(ops.device)
    gz, dx = ops.linear_bwd(g, y, w)
    gz_p, dx_p = ops.linear_bwd(g, y, w, flags=PLAIN)
    assert torch.equal(gz, gz_p) and torch.equal(dx, dx_p)
    dx64 = gz.double() @ w.double()
    scale = gz.double().abs() @ w.double().abs()
    e_lib = float(((torch.matmul(gz, w).double() - dx64).abs() / scale).max())
    e_own = float(((dx.double() - dx64).abs() / scale).max())
    print("ragged bwd: pn_linear_bwd %.3e  library %.3e" % (e_own, e_lib))
    assert e_own <= 1.5 * e_lib


def test_twenty_launches_back_to_back_give_the_first_ones_bits():
    """A cheap screen for an LDS read or store that no barrier orders (such a race passes most single runs: the order is argued in
    pipelined_slabs, not here).  Three output buffers in rotation, one comparison on the stream between two launches, no host wait."""
    rows, width, k = 384, 256, 320
    ops = _ops(rows * k)
    x, w, b = _operands("normal", rows, k, width, 21, ops.device)
    ys = [torch.empty(rows, width, device=ops.device) for _ in range(3)]
    first = ops.linear_fwd(x, w, b, True).clone()
    assert torch.equal(first, ops.linear_fwd(x, w, b, True))
    same = []
    for i in range(20):
        ops.linear_fwd(x, w, b, True, ys[i % 3])
        same.append(torch.eq(ys[i % 3], first).all())
    assert bool(torch.stack(same).all())
    g, wt, _ = _operands("normal", rows, k, width, 22, ops.device)
    wb = wt.t().contiguous()
    a = torch.tanh(g.roll(1, 0))
    gz0, dx0 = (t.clone() for t in ops.linear_bwd(g, a, wb))
    gzs = [torch.empty_like(gz0) for _ in range(3)]
    dxs = [torch.empty_like(dx0) for _ in range(3)]
    same = []
    for i in range(20):
        ops.linear_bwd(g, a, wb, gzs[i % 3], dxs[i % 3])
        same.append(torch.eq(gzs[i % 3], gz0).all() & torch.eq(dxs[i % 3], dx0).all())
    assert bool(torch.stack(same).all())
