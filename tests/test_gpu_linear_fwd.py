"""-m gpu: pn_linear_fwd (csrc/pn_linear.hip), y = act(x w^T + b) in one launch, through HipVecOps against float64.

Shapes: rows 256 / 320 (ragged: no multiple of the 64-row tile) / 384; (out_f, in_f) = (64, 64) one 128-wide tile half empty, (192, 64)
two tiles of which the second is half empty, (64, 192) six K slabs, (128, 256) one full tile, eight slabs; bias present and absent;
act = identity and tanh.

The bar of the random-operand case is the library path's own error, torch.tanh(F.linear(x, w, b)) in fp32 on the same operands, in
the same measure -- max |y - y64| / (sum_k |x w| + |b|) -- times MARGIN = 2:
  * the product: six of the nine bf16 x bf16 terms, fp32 accumulation: 5.7e-8 of sum |x w| at K = 512 against 1.0e-7 for an fp32 fmaf
    chain (tools/mb_wgrad_bf16x3.hip) -- no margin needed for it;
  * the activation: tanhf of the device library, documented at up to 2 ulp, where the library path's tanh rounds within about 1: twice
    the error on the activation's share, hence 2.
Measured on MI355X, worst over the 48 cases of this file: identity pn_linear_fwd 1.43e-7 against the library's 2.98e-7 (worst ratio within
a case 0.66), tanh 9.9e-8 against 1.74e-7 (worst ratio 0.78); exact operands with tanh: 2.9e-8 from float64 (half an ulp)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import require_gpu

pytestmark = pytest.mark.gpu

ROWS = [256, 320, 384]
SHAPES = [(64, 64), (192, 64), (64, 192), (128, 256)]
MARGIN = 2.0
ULP = 2.0 ** -24            # the spacing of fp32 in [0.5, 1): the largest ulp a tanh value has


def _ops(rows, in_f):
    from pnode_amd._vecops import HipVecOps
    return HipVecOps(require_gpu(), torch.float32, rows * in_f)


def _variants():
    return [(bias, tanh) for bias in (True, False) for tanh in (False, True)]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("out_f,in_f", SHAPES)
def test_exact_operands_give_the_float64_result(rows, out_f, in_f):
    """Small integers: every product and every partial sum is exact in bf16 x bf16 -> fp32, whatever the order."""
    ops = _ops(rows, in_f)
    g = torch.Generator().manual_seed(rows + 7 * out_f + in_f)
    x = torch.randint(-4, 5, (rows, in_f), generator=g).float().to(ops.device)
    w = torch.randint(-4, 5, (out_f, in_f), generator=g).float().to(ops.device)
    b = torch.randint(-8, 9, (out_f,), generator=g).float().to(ops.device)
    # (rows of zeros: z = b, tanh values away from saturation as well)
    x[::5] = 0
    for bias, tanh in _variants():
        z64 = F.linear(x.double(), w.double(), b.double() if bias else None)
        y = ops.linear_fwd(x, w, b if bias else None, tanh)
        if not tanh:
            assert torch.equal(y, z64.float()), (bias, float((y.double() - z64).abs().max()))
        else:
            # the argument is exact: what is left is tanhf's own error (2 ulp) and the rounding of the float64 value (half an ulp)
            err = (y.double() - torch.tanh(z64)).abs().max()
            print("exact operands, tanh: max error %.3e" % float(err))
            assert float(err) <= 2.5 * ULP
            lib = torch.tanh(z64.float())
            assert float((y - lib).abs().max()) <= 3.5 * ULP      # (the library's tanh: within 1 ulp of its own)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("out_f,in_f", SHAPES)
def test_random_operands_are_as_close_to_float64_as_the_library_path(rows, out_f, in_f):
    ops = _ops(rows, in_f)
    g = torch.Generator().manual_seed(3 * rows + out_f + 11 * in_f)
    x = torch.randn(rows, in_f, generator=g).to(ops.device)
    w = (torch.randn(out_f, in_f, generator=g) / in_f ** 0.5).to(ops.device)
    b = torch.randn(out_f, generator=g).to(ops.device)
    for bias, tanh in _variants():
        bb = b if bias else None
        z64 = F.linear(x.double(), w.double(), None if bb is None else bb.double())
        scale = x.double().abs() @ w.double().abs().t() + (b.double().abs() if bias else 0.0)
        ref = torch.tanh(z64) if tanh else z64
        lib = F.linear(x, w, bb)
        lib = torch.tanh(lib) if tanh else lib
        y = ops.linear_fwd(x, w, bb, tanh)
        e_lib = float(((lib.double() - ref).abs() / scale).max())
        e_own = float(((y.double() - ref).abs() / scale).max())
        print("rows %d out %d in %d bias %d tanh %d: pn_linear_fwd %.3e  library %.3e  ratio %.2f" % (rows, out_f, in_f, bias, tanh, e_own, e_lib, e_own / e_lib))
        assert e_own <= MARGIN * e_lib, (bias, tanh, e_own, e_lib)


def test_saturation_nan_and_inf_stay_in_their_rows_and_launches_repeat_bitwise():
    rows, out_f, in_f = 320, 192, 64
    ops = _ops(rows, in_f)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, in_f, generator=g).to(ops.device)
    w = (torch.randn(out_f, in_f, generator=g) / in_f ** 0.5).to(ops.device)
    b = torch.randn(out_f, generator=g).to(ops.device)
    clean = ops.linear_fwd(x, w, b, True)
    assert torch.equal(clean, ops.linear_fwd(x, w, b, True))
    assert bool(torch.isfinite(clean).all())
    # rows that drive |z| to 50, 1e4 and 1e30: exactly +-1
    x2 = x.clone()
    sgn = torch.sign(w[0])
    for r, s in ((3, 50.0), (100, -50.0), (257, 1e4), (319, -1e30)):
        x2[r] = sgn * (s / float(w[0].abs().sum()))
    w2 = w.clone()
    w2[1:] = w[0]                                   # every column sees the same z (+ its bias, |b| < 6)
    y = ops.linear_fwd(x2, w2, b, True)
    z64 = F.linear(x2.double(), w2.double(), b.double())
    for r in (3, 100, 257, 319):
        assert float(z64[r].abs().min()) >= 40.0
        assert torch.equal(y[r], torch.sign(z64[r]).float()), r
    assert not bool(torch.isnan(y).any())
    # NaN and Inf in X: non-finite values in their own rows only (the split of an infinite operand is inf - inf: NaN, as pn_linear_wgrad)
    x3 = x.clone()
    x3[17, 5] = float("nan")
    x3[300, 63] = float("inf")
    for tanh in (False, True):
        base = ops.linear_fwd(x, w, b, tanh)
        y = ops.linear_fwd(x3, w, b, tanh)
        bad = torch.zeros(rows, dtype=torch.bool, device=ops.device)
        bad[17] = bad[300] = True
        assert torch.equal(y[~bad], base[~bad])
        assert bool(torch.isnan(y[17]).all())
        assert not bool(torch.isfinite(y[300]).any()) or tanh
        assert bool((torch.isnan(y[300]) | (y[300].abs() == 1.0) | torch.isinf(y[300])).all())


@pytest.mark.parametrize("rows,out_f,in_f", [(255, 64, 64), (256, 64, 80), (256, 64, 32), (256, 96, 64)])
def test_unsupported_shapes_are_reported_and_never_launch(rows, out_f, in_f):
    from pnode_amd._lib import PnError
    ops = _ops(rows, in_f)
    assert not ops.linear_fwd_supported(rows, out_f, in_f)
    x = torch.ones(rows, in_f, device=ops.device)
    w = torch.ones(out_f, in_f, device=ops.device)
    y = torch.full((rows, out_f), 7.0, device=ops.device)
    with pytest.raises(PnError):
        ops.linear_fwd(x, w, None, True, y)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    ops64 = _ops(256, 64)
    ops64.code = 1                                  # (the fp64 state's code)
    assert not ops64.linear_fwd_supported(256, 64, 64)
