"""-m gpu: the ReLU forms of pn_linear_fwd (PN_ACT_RELU) and pn_linear_bwd_act (csrc/pn_linear.hip), through HipVecOps.

Shapes (rows, out_f, in_f), the smallest at which each form can go wrong.  Forward (K = in_f): 256 x 128 x 64 aligned, two slabs:
pipelined, and the same with PN_LINEAR_FORM_PLAIN; 256 x 128 x 96 three slabs -- an odd number: the plain loop; 300 x 192 x 64 ragged in
rows and columns; each with and without a bias.  Backward (K = out_f, columns = in_f): 256 x 64 x 128, the same plain, 256 x 96 x 128,
300 x 64 x 192.

The contract is bits.  Forward: y under PN_ACT_RELU is relu of the y under PN_ACT_IDENTITY in the same form, value for value -- the
epilogue is a compare on the biased sum; so the identity's bound against float64 carries over (ReLU is 1-Lipschitz): CHECK_TOL = 1e-6 of
sum |x w| + |b|, the engine's self-check bar.  Backward: gz is aten.threshold_backward(g, a, 0) bit for bit (no arithmetic touches g), and
dx has the bits of pn_linear_dx fed that gz (the prologue sits in front of the bare body), in every form."""
import pytest
import torch

import _linear_tile_cases as tc
from conftest import require_gpu

pytestmark = pytest.mark.gpu

PLAIN = 1                             # PN_LINEAR_FORM_PLAIN
CHECK_TOL = 1e-6
FWD_CASES = [(256, 128, 64, 0), (256, 128, 64, PLAIN), (256, 128, 96, 0), (300, 192, 64, 0)]
BWD_CASES = [(256, 64, 128, 0), (256, 64, 128, PLAIN), (256, 96, 128, 0), (300, 64, 192, 0)]


def _ops():
    from pnode_amd import _lib, _linearfwd
    from pnode_amd._vecops import HipVecOps
    assert _lib.PN_LINEAR_FORM_PLAIN == PLAIN and _linearfwd.CHECK_TOL == CHECK_TOL and HipVecOps.linear_relu is True
    return HipVecOps(require_gpu(), torch.float32, 300 * 192)


def _randn(rows, cols, seed):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


def test_the_cases_reach_every_instantiation():
    for cases, width, k in ((FWD_CASES, 1, 2), (BWD_CASES, 2, 1)):
        kinds = set()
        for case in cases:
            rows, flags = case[0], case[3]
            if not tc.is_aligned(rows, case[width]):
                kinds.add("ragged")
            else:
                kinds.add("pipelined" if tc.pipelines(case[k]) and not flags else "plain")
        assert kinds == {"ragged", "pipelined", "plain"}


# ------------------------------------------------------------------------------------------------------------------------- forward
_FWD = {}


def _forward(rows, out_f, in_f, flags, bias):
    """Operands N(0, 1) -- column 3 of w zero (with a zero bias), the bias of column 5 -1e3 -- and the ReLU and identity results."""
    key = (rows, out_f, in_f, flags, bias)
    if key not in _FWD:
        ops = _ops()
        seed = tc.case_seed(rows, out_f, in_f)
        x, w = _randn(rows, in_f, seed).to(ops.device), _randn(out_f, in_f, seed + 17)
        w[3] = 0.0
        w = w.to(ops.device)
        b = None
        if bias:
            b = _randn(1, out_f, seed + 5).view(-1)
            b[3], b[5] = 0.0, -1e3
            b = b.to(ops.device)
        y = ops.linear_fwd(x, w, b, False, flags=flags, act="relu")
        ident = ops.linear_fwd(x, w, b, False, flags=flags)
        assert ops.linear_fwd_supported(rows, out_f, in_f) and y.shape == (rows, out_f) and y.dtype == torch.float32
        _FWD[key] = (ops, x, w, b, y, ident)
    return _FWD[key]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_relu_forward_is_relu_of_the_identity_forward_value_for_value(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, ident = _forward(rows, out_f, in_f, flags, bias)
    assert bool(torch.isfinite(ident).all()) and bool((ident < 0).any()) and bool((ident > 0).any())
    assert torch.equal(y, torch.relu(ident))
    # the positive values keep their bits, everything else is +0
    pos = ident > 0
    assert torch.equal(y[pos].view(torch.int32), ident[pos].view(torch.int32)) and bool((y[~pos].view(torch.int32) == 0).all())
    # "act" by name is what the positional flag says
    assert torch.equal(ops.linear_fwd(x, w, b, True, flags=flags), ops.linear_fwd(x, w, b, False, flags=flags, act="tanh"))
    assert torch.equal(ident, ops.linear_fwd(x, w, b, True, flags=flags, act="identity"))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_relu_forward_against_float64_within_the_self_check_bar(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, _ = _forward(rows, out_f, in_f, flags, bias)
    z = tc.forward64(x, w, b)
    scale = x.double().abs() @ w.double().abs().t()
    if b is not None:
        scale = scale + b.double().abs()
    err = (y.double() - torch.relu(z)).abs()
    ok = scale > 0
    worst = float((err[ok] / scale[ok]).max())
    print("rows %d out %d in %d flags %d bias %s: max |y - relu(z64)| / (sum |x w| + |b|) = %.3e" % (rows, out_f, in_f, flags, bias, worst))
    assert bool((err <= CHECK_TOL * scale).all()), worst


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_a_zero_column_and_a_far_negative_bias_give_plus_zero(rows, out_f, in_f, flags, bias):
    _, _, _, b, y, _ = _forward(rows, out_f, in_f, flags, bias)
    assert bool((y[:, 3].view(torch.int32) == 0).all())
    if bias:
        assert float(b[5]) == -1e3 and bool((y[:, 5].view(torch.int32) == 0).all())


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_a_nan_row_of_x_gives_a_nan_row_and_leaves_every_other_rows_bits(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, _ = _forward(rows, out_f, in_f, flags, bias)
    x2 = x.clone()
    x2[rows - 2] = float("nan")
    y2 = ops.linear_fwd(x2, w, b, False, flags=flags, act="relu")
    others = torch.ones(rows, dtype=torch.bool, device=ops.device)
    others[rows - 2] = False
    assert bool(torch.isnan(y2[rows - 2]).all())
    assert torch.equal(y2[others].view(torch.int32), y[others].view(torch.int32))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_two_forward_launches_give_the_same_bits_inside_their_guards(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, _ = _forward(rows, out_f, in_f, flags, bias)
    buf, view = tc.guarded(rows, out_f, ops.device)
    out = ops.linear_fwd(x, w, b, False, view, flags=flags, act="relu")
    torch.cuda.synchronize()
    assert out is view and tc.guards_untouched(buf, rows)
    assert torch.equal(view.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ backward
_BWD = {}


def _signs(rows, k, seed, nans):
    """The pair's output as the kernel may meet it: positives, exact zeros, -0.0, negatives (a ReLU gives none: the rule is
    threshold_backward's all the same) and, with `nans`, a few NaNs."""
    a = _randn(rows, k, seed)
    pick = torch.randint(0, 8, (rows, k), generator=torch.Generator().manual_seed(seed + 1))
    a[pick == 0] = 0.0
    a[pick == 1] = -0.0
    if nans:
        a[pick == 2] = float("nan")
        a[0, 0], a[rows - 1, k - 1] = float("nan"), float("nan")
    a[1, 1], a[2, 2], a[3, 3], a[4, 4] = 0.0, -0.0, -1.0, 1.0
    return a


def _backward(rows, out_f, in_f, flags):
    key = (rows, out_f, in_f, flags)
    if key not in _BWD:
        ops = _ops()
        seed = tc.case_seed(rows, in_f, out_f)
        g = _randn(rows, out_f, seed).to(ops.device)
        w = (_randn(out_f, in_f, seed + 17) * out_f ** -0.5).to(ops.device)
        a = _signs(rows, out_f, seed + 3, False).to(ops.device)
        gbuf, gz = tc.guarded(rows, out_f, ops.device)
        dbuf, dx = tc.guarded(rows, in_f, ops.device)
        out = ops.linear_bwd(g, a, w, gz, dx, flags=flags, act="relu")
        torch.cuda.synchronize()
        assert out[0] is gz and out[1] is dx and ops.linear_bwd_supported(rows, out_f, in_f)
        _BWD[key] = (ops, g, a, w, gbuf, gz, dbuf, dx)
    return _BWD[key]


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_gz_is_threshold_backward_bit_for_bit_and_a_nan_in_a_lets_g_through(rows, out_f, in_f, flags):
    ops, g, a, w, _, gz, _, _ = _backward(rows, out_f, in_f, flags)
    want = torch.ops.aten.threshold_backward(g, a, 0)
    assert torch.equal(gz, want) and torch.equal(gz.view(torch.int32), want.view(torch.int32))
    a2 = _signs(rows, out_f, tc.case_seed(rows, in_f, out_f) + 3, True).to(ops.device)
    nan = torch.isnan(a2)
    assert int(nan.sum()) > 2 and bool((a2 == 0).any()) and bool((a2 < 0).any()) and bool((a2 > 0).any())
    assert bool((a2.view(torch.int32) == -2 ** 31).any())                  # -0.0
    gz2, _ = ops.linear_bwd(g, a2, w, flags=flags, act="relu")
    want2 = torch.ops.aten.threshold_backward(g, a2, 0)
    assert torch.equal(gz2.view(torch.int32), want2.view(torch.int32))
    assert torch.equal(gz2[nan].view(torch.int32), g[nan].view(torch.int32))
    zero = (a2 <= 0)
    assert bool((gz2[zero].view(torch.int32) == 0).all())                   # +0 also where a is -0.0 or g is negative


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_dx_has_the_bits_of_pn_linear_dx_fed_gz(rows, out_f, in_f, flags):
    ops, g, a, w, _, gz, _, dx = _backward(rows, out_f, in_f, flags)
    assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(g).any())
    want = ops.linear_dx(gz.contiguous(), w, flags=flags)
    assert dx.shape == (rows, in_f) and torch.equal(dx.view(torch.int32), want.view(torch.int32)), int((dx != want).sum())
    # ... and is as far from float64 as the engine's self-check allows at most
    ref = gz.double() @ w.double()
    scale = gz.double().abs() @ w.double().abs()
    assert bool(((dx.double() - ref).abs() <= CHECK_TOL * scale).all())


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_the_sentinels_around_gz_and_dx_stay_and_a_second_launch_gives_the_same_bits(rows, out_f, in_f, flags):
    ops, g, a, w, gbuf, gz, dbuf, dx = _backward(rows, out_f, in_f, flags)
    assert tc.guards_untouched(gbuf, rows) and tc.guards_untouched(dbuf, rows)
    gbuf2, gz2 = tc.guarded(rows, out_f, ops.device)
    dbuf2, dx2 = tc.guarded(rows, in_f, ops.device)
    ops.linear_bwd(g, a, w, gz2, dx2, flags=flags, act="relu")
    torch.cuda.synchronize()
    assert tc.guards_untouched(gbuf2, rows) and tc.guards_untouched(dbuf2, rows)
    assert torch.equal(gz2.view(torch.int32), gz.view(torch.int32)) and torch.equal(dx2.view(torch.int32), dx.view(torch.int32))


def _act(ops, g, a, w, act, gz, dx, flags, rows=None, out_f=None, in_f=None):
    """pn_linear_bwd_act as it is exported; tensors or raw addresses."""
    def ptr(v):
        return v.data_ptr() if isinstance(v, torch.Tensor) else v
    rows = g.shape[0] if rows is None else rows
    out_f = w.shape[0] if out_f is None else out_f
    in_f = w.shape[1] if in_f is None else in_f
    return ops.lib.pn_linear_bwd_act(ops.stream(), ops.code, rows, out_f, in_f, ptr(g), ptr(a), ptr(w), act, ptr(gz), ptr(dx), flags)


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_pn_linear_bwd_act_with_tanh_is_pn_linear_bwd_form_bit_for_bit(rows, out_f, in_f, flags):
    from pnode_amd import _lib
    ops, g, _, w, _, _, _, _ = _backward(rows, out_f, in_f, flags)
    a = torch.tanh(_randn(rows, out_f, 11)).to(ops.device)
    gz_f, dx_f = ops.linear_bwd(g, a, w, flags=flags)
    gz, dx = torch.empty_like(gz_f), torch.empty_like(dx_f)
    assert _act(ops, g, a, w, _lib.PN_ACT_TANH, gz, dx, flags) == 0
    torch.cuda.synchronize()
    assert torch.equal(gz.view(torch.int32), gz_f.view(torch.int32)) and torch.equal(dx.view(torch.int32), dx_f.view(torch.int32))


@pytest.mark.parametrize("flags", [0, PLAIN])
def test_refused_calls_return_nonzero_and_leave_the_outputs_untouched(flags):
    from pnode_amd import _lib
    from pnode_amd._lib import PnError
    ops = _ops()
    RELU = _lib.PN_ACT_RELU
    rows, out_f, in_f = 256, 64, 128
    g = torch.full((rows, out_f), 7.0, device=ops.device)
    a = torch.full((rows, out_f), 1.0, device=ops.device)
    w = torch.full((out_f, in_f), 5.0, device=ops.device)
    gbuf, gz = tc.guarded(rows, out_f, ops.device)
    dbuf, dx = tc.guarded(rows, in_f, ops.device)

    def untouched():
        torch.cuda.synchronize()
        words = (gbuf.view(torch.int32), dbuf.view(torch.int32))
        return all(bool((v == tc.SENTINEL).all()) for v in words) and bool((g == 7.0).all()) and bool((a == 1.0).all()) and bool((w == 5.0).all())

    def last():
        return ops.lib.pn_last_error().decode()

    assert _act(ops, g, a, w, _lib.PN_ACT_IDENTITY, gz, dx, flags) != 0 and "use pn_linear_dx" in last() and untouched()
    assert _act(ops, g, a, w, 7, gz, dx, flags) != 0 and "act is PN_ACT_TANH or PN_ACT_RELU" in last() and untouched()
    assert _act(ops, g, a, w, RELU, gz, dx, flags | 2) != 0 and "pn_linear_bwd_act: unknown flag" in last() and untouched()
    # gz is g; dx is gz (256 x 64 x 64: the two have one shape)
    assert _act(ops, g, a, w, RELU, g, dx, flags) != 0 and "gz must not alias" in last() and untouched()
    w64 = torch.full((64, 64), 5.0, device=ops.device)
    assert _act(ops, g, a, w64, RELU, gz, gz, flags) != 0 and "dx must not alias" in last() and untouched()
    assert _act(ops, g, a, w64, RELU, gz, gz.data_ptr() + 4 * rows * 64 - 16, flags) != 0 and "dx must not alias" in last() and untouched()
    # a pointer off 16 bytes: each operand in turn
    for k in range(5):
        args = [g, a, w, gz, dx]
        args[k] = args[k].data_ptr() + 4
        assert _act(ops, args[0], args[1], args[2], RELU, args[3], args[4], flags, rows, out_f, in_f) != 0 and "16-byte aligned" in last()
    assert untouched()
    # shapes outside pn_linear_bwd_supported: 128 rows, K = 48, 100 columns; an fp64 state
    for r, o, i in ((128, out_f, in_f), (rows, 48, in_f), (rows, out_f, 100)):
        assert not ops.linear_bwd_supported(r, o, i)
        assert _act(ops, g, a, w, RELU, gz, dx, flags, r, o, i) != 0 and "unsupported dtype or shape" in last()
    assert ops.lib.pn_linear_bwd_act(ops.stream(), 1, rows, out_f, in_f, g.data_ptr(), a.data_ptr(), w.data_ptr(), RELU, gz.data_ptr(),
                                     dx.data_ptr(), flags) != 0 and "unsupported dtype or shape" in last()
    assert untouched()
    # the backend refuses an activation it does not know, by name, before any launch
    with pytest.raises(PnError, match="tanh or relu"):
        ops.linear_bwd(g, a, w, gz, dx, flags=flags, act="identity")
    with pytest.raises(PnError, match="identity, tanh or relu"):
        ops.linear_fwd(g, w.t().contiguous(), None, False, flags=flags, act="gelu")
    assert untouched()
    # and the same operands, not aliased, go through: a > 0 everywhere, so gz is g and dx is 64 * 7 * 5
    assert _act(ops, g, a, w, RELU, gz, dx, flags) == 0
    torch.cuda.synchronize()
    assert bool((gz == 7.0).all()) and bool((dx == out_f * 7.0 * 5.0).all()) and tc.guards_untouched(gbuf, rows) and tc.guards_untouched(dbuf, rows)
