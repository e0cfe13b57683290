"""-m gpu: the Sigmoid forms of pn_linear_fwd (PN_ACT_SIGMOID) and pn_linear_bwd_act (csrc/pn_linear.hip), through HipVecOps.

Shapes (rows, out_f, in_f): the cases of tests/test_gpu_linear_relu.py.  Forward (K = in_f): 256 x 128 x 64 aligned, two slabs:
pipelined, and the same with PN_LINEAR_FORM_PLAIN; 256 x 128 x 96 three slabs -- an odd number: the plain loop; 300 x 192 x 64 ragged in
rows and columns; each with and without a bias.  Backward (K = out_f, columns = in_f): 256 x 64 x 128, the same plain, 256 x 96 x 128,
300 x 64 x 192.

The arithmetic is not exact, so the contract is bounds plus the same bits across forms.  ULP = 2^-24, the spacing of fp32 in [0.5, 1).
Forward, y = 1 / (1 + e), e = expf(-z), on the identity kernel's z, y <= 1: expf within 1 ulp -- 2 ULP relative -- moves y by
2 ULP y (1 - y) <= ULP / 2; the rounded add, ULP relative, by ULP y <= ULP; the correctly rounded division by half the spacing of y,
<= ULP / 2: 2 ULP in all, 2.5 with room; torch.sigmoid adds its own 1 ULP.  Backward, gz = g * fmaf(-a, a, a): two roundings, each ULP
relative, 2.5 ULP relative with room for the second-order term.  dx has the bits of pn_linear_dx fed that gz.

Random operands, error against float64 in the measure |y - y64| / (sum |x w| + |b|), pn_linear_fwd against torch.sigmoid(F.linear) on the
same operands (MARGIN = 2, the method of tests/test_gpu_linear_fwd.py).  Measured on MI355X over the eight cases: pn_linear_fwd 2.5e-8 to
3.1e-8 against the library's 3.6e-8 to 4.6e-8, worst ratio within a case 0.86; |y - sigma(y_id)| at most 1.45 ULP; on exact operands 1.43
ULP from float64 and torch.sigmoid's bits; |gz - g a (1 - a)| at most 1.82 ULP relative."""
import pytest
import torch
import torch.nn.functional as F

import _linear_tile_cases as tc
from conftest import require_gpu

pytestmark = pytest.mark.gpu

PLAIN = 1                             # PN_LINEAR_FORM_PLAIN
ULP = 2.0 ** -24
MARGIN = 2.0
CHECK_TOL = 1e-6
FWD_CASES = [(256, 128, 64, 0), (256, 128, 64, PLAIN), (256, 128, 96, 0), (300, 192, 64, 0)]
BWD_CASES = [(256, 64, 128, 0), (256, 64, 128, PLAIN), (256, 96, 128, 0), (300, 64, 192, 0)]
ONE_ROW, ZERO_ROW = 5, 6              # rows of the exact operands driven to z >= 40 and to z <= -110


def _ops():
    from pnode_amd import _lib, _linearfwd
    from pnode_amd._vecops import HipVecOps
    assert _lib.PN_LINEAR_FORM_PLAIN == PLAIN and _linearfwd.CHECK_TOL == CHECK_TOL and HipVecOps.linear_sigmoid is True
    assert _lib.PN_ACT_SIGMOID == 4
    return HipVecOps(require_gpu(), torch.float32, 300 * 192)


def _randn(rows, cols, seed):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


def _randint(lo, hi, rows, cols, seed):
    return torch.randint(lo, hi + 1, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


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
    """Operands N(0, 1), w scaled by in_f^-1/2 (z of a few units: sigma outside its saturation), and the Sigmoid and identity results."""
    key = (rows, out_f, in_f, flags, bias)
    if key not in _FWD:
        ops = _ops()
        seed = tc.case_seed(rows, out_f, in_f)
        x = _randn(rows, in_f, seed).to(ops.device)
        w = (_randn(out_f, in_f, seed + 17) * in_f ** -0.5).to(ops.device)
        b = _randn(1, out_f, seed + 5).view(-1).to(ops.device) if bias else None
        y = ops.linear_fwd(x, w, b, False, flags=flags, act="sigmoid")
        ident = ops.linear_fwd(x, w, b, False, flags=flags)
        assert ops.linear_fwd_supported(rows, out_f, in_f) and y.shape == (rows, out_f) and y.dtype == torch.float32
        _FWD[key] = (ops, x, w, b, y, ident)
    return _FWD[key]


def _exact(rows, out_f, in_f, flags, bias):
    """Small-integer operands: x in quarters of -4 .. 4, w in quarters of -2 .. 2, b in quarters of -8 .. 8 -- every product a multiple of
    1/16 below 1, every sum exact in fp32 in any order and in the split.  Row ONE_ROW of x is +4 and row ZERO_ROW -8 against column 0
    and 1 of w set to +1/4 throughout: z = in_f + b >= 62 there, z = -2 in_f + b <= -126."""
    key = ("exact", rows, out_f, in_f, flags, bias)
    if key not in _FWD:
        ops = _ops()
        seed = tc.case_seed(rows, out_f, in_f)
        x, w = _randint(-4, 4, rows, in_f, seed) / 4, _randint(-2, 2, out_f, in_f, seed + 17) / 4
        x[ONE_ROW], x[ZERO_ROW] = 4.0, -8.0
        w[0], w[1] = 0.25, 0.25
        b = _randint(-8, 8, 1, out_f, seed + 5).view(-1) / 4 if bias else None
        x, w, b = x.to(ops.device), w.to(ops.device), None if b is None else b.to(ops.device)
        y = ops.linear_fwd(x, w, b, False, flags=flags, act="sigmoid")
        ident = ops.linear_fwd(x, w, b, False, flags=flags)
        _FWD[key] = (ops, x, w, b, y, ident)
    return _FWD[key]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_sigmoid_forward_is_sigma_of_the_identity_forward_to_two_and_a_half_ulp(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, ident = _forward(rows, out_f, in_f, flags, bias)
    assert bool(torch.isfinite(ident).all()) and bool((ident < 0).any()) and bool((ident > 0).any()) and float(ident.abs().max()) < 15.0
    err = (y.double() - torch.sigmoid(ident.double())).abs()
    print("rows %d out %d in %d flags %d bias %s: max |y - sigma(y_id)| = %.2f ULP" % (rows, out_f, in_f, flags, bias, float(err.max()) / ULP))
    assert bool((err <= 2.5 * ULP).all()), float(err.max()) / ULP
    assert bool((y > 0).all()) and bool((y < 1).all())
    # "act" by name is what the positional flag says
    assert torch.equal(ident, ops.linear_fwd(x, w, b, True, flags=flags, act="identity"))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_exact_operands_against_float64_and_against_torch_sigmoid_of_the_exact_z(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, ident = _exact(rows, out_f, in_f, flags, bias)
    z64 = tc.forward64(x, w, b)
    z = z64.float()
    assert torch.equal(z.double(), z64) and torch.equal(ident, z)          # the premise: z is exact, and the identity kernel gives it
    e64 = (y.double() - torch.sigmoid(z64)).abs()
    e32 = (y.double() - torch.sigmoid(z).double()).abs()
    print("rows %d out %d in %d flags %d bias %s: max |y - sigma64(z)| = %.2f ULP, |y - torch.sigmoid(z)| = %.2f ULP"
          % (rows, out_f, in_f, flags, bias, float(e64.max()) / ULP, float(e32.max()) / ULP))
    assert bool((e64 <= 2.5 * ULP).all()) and bool((e32 <= 3.5 * ULP).all())
    # never above 1, never negative; nothing is 0 down to z = -80, nothing is 1 up to z = 15 (sigma(15) = 1 - 3.06e-7 is below 1 in fp32)
    assert bool((y <= 1).all()) and bool((y >= 0).all()) and bool((y[z >= -80] > 0).all()) and bool((y[z <= 15] < 1).all())
    assert bool((z.abs() < 15).any())


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_saturation_is_exactly_one_and_exactly_plus_zero(rows, out_f, in_f, flags, bias):
    _, _, _, _, y, ident = _exact(rows, out_f, in_f, flags, bias)
    assert float(ident[ONE_ROW, :2].min()) >= 40.0 and float(ident[ZERO_ROW, :2].max()) <= -110.0
    assert bool((y[ONE_ROW, :2] == 1.0).all()) and bool((y[ZERO_ROW, :2].view(torch.int32) == 0).all())
    # ... and wherever else the exact z is that far out
    assert bool((y[ident >= 40.0] == 1.0).all()) and bool((y[ident <= -110.0].view(torch.int32) == 0).all())


def test_random_operands_against_float64_within_twice_the_library_pairs_own_error():
    """Measured on MI355X: worst ratio own / library over the eight cases 0.86 (2.506e-8 .. 3.128e-8 against 3.616e-8 .. 4.575e-8)."""
    worst = 0.0
    for rows, out_f, in_f, flags in FWD_CASES:
        for bias in (True, False):
            ops, x, w, b, y, _ = _forward(rows, out_f, in_f, flags, bias)
            ref = torch.sigmoid(tc.forward64(x, w, b))
            scale = x.double().abs() @ w.double().abs().t()
            if b is not None:
                scale = scale + b.double().abs()
            lib = torch.sigmoid(F.linear(x, w, b))
            e_own = float(((y.double() - ref).abs() / scale).max())
            e_lib = float(((lib.double() - ref).abs() / scale).max())
            worst = max(worst, e_own / e_lib)
            print("rows %d out %d in %d flags %d bias %d: pn_linear_fwd %.3e  library %.3e  ratio %.2f" % (rows, out_f, in_f, flags, bias, e_own, e_lib, e_own / e_lib))
            assert e_own <= MARGIN * e_lib, (rows, out_f, in_f, flags, bias, e_own, e_lib)
    print("worst ratio %.2f" % worst)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_a_nan_row_of_x_gives_a_nan_row_and_leaves_every_other_rows_bits(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, _ = _forward(rows, out_f, in_f, flags, bias)
    x2 = x.clone()
    x2[rows - 2] = float("nan")
    y2 = ops.linear_fwd(x2, w, b, False, flags=flags, act="sigmoid")
    others = torch.ones(rows, dtype=torch.bool, device=ops.device)
    others[rows - 2] = False
    assert bool(torch.isnan(y2[rows - 2]).all())
    assert torch.equal(y2[others].view(torch.int32), y[others].view(torch.int32))


@pytest.mark.parametrize("bias", [True, False])
def test_the_forward_has_the_same_bits_in_every_form(bias):
    ops, x, w, b, y, _ = _forward(256, 128, 64, 0, bias)
    _, x1, w1, b1, y_plain, _ = _forward(256, 128, 64, PLAIN, bias)
    assert torch.equal(x, x1) and torch.equal(w, w1) and torch.equal(y.view(torch.int32), y_plain.view(torch.int32))
    # the ragged body: 300 rows whose first 256 are these -- a row of y depends on that row of x, on w and on b alone
    x300 = torch.cat([x, _randn(44, 64, 99).to(ops.device)])
    y300 = ops.linear_fwd(x300, w, b, False, act="sigmoid")
    assert not tc.is_aligned(300, 128) and torch.equal(y300[:256].view(torch.int32), y.view(torch.int32))
    assert bool(((y300[256:] > 0) & (y300[256:] < 1)).all())


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_two_forward_launches_give_the_same_bits_inside_their_guards(rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, _ = _forward(rows, out_f, in_f, flags, bias)
    buf, view = tc.guarded(rows, out_f, ops.device)
    out = ops.linear_fwd(x, w, b, False, view, flags=flags, act="sigmoid")
    torch.cuda.synchronize()
    assert out is view and tc.guards_untouched(buf, rows)
    assert torch.equal(view.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ backward
_BWD = {}


def _outputs(rows, k, seed, nans):
    """The pair's output as the kernel may meet it: values of (0, 1), exact zeros and ones and, with `nans`, a few NaNs."""
    a = torch.sigmoid(2.0 * _randn(rows, k, seed))
    assert bool(((a > 0) & (a < 1)).all())
    pick = torch.randint(0, 8, (rows, k), generator=torch.Generator().manual_seed(seed + 1))
    a[pick == 0] = 0.0
    a[pick == 1] = 1.0
    if nans:
        a[16:24][pick[16:24] == 2] = float("nan")                 # (eight rows of them; the other rows stay clean)
        a[0, 0], a[rows - 1, k - 1] = float("nan"), float("nan")
    a[1, 1], a[2, 2] = 0.0, 1.0
    return a


def _backward(rows, out_f, in_f, flags):
    key = (rows, out_f, in_f, flags)
    if key not in _BWD:
        ops = _ops()
        seed = tc.case_seed(rows, in_f, out_f)
        g = _randn(rows, out_f, seed)
        g[g.abs() < 1e-3] = 1e-3                   # (the normal range, well away from a product that underflows)
        g = g.to(ops.device)
        w = (_randn(out_f, in_f, seed + 17) * out_f ** -0.5).to(ops.device)
        a = _outputs(rows, out_f, seed + 3, False).to(ops.device)
        gbuf, gz = tc.guarded(rows, out_f, ops.device)
        dbuf, dx = tc.guarded(rows, in_f, ops.device)
        out = ops.linear_bwd(g, a, w, gz, dx, flags=flags, act="sigmoid")
        torch.cuda.synchronize()
        assert out[0] is gz and out[1] is dx and ops.linear_bwd_supported(rows, out_f, in_f)
        _BWD[key] = (ops, g, a, w, gbuf, gz, dbuf, dx)
    return _BWD[key]


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_gz_is_g_a_one_minus_a_to_two_roundings_and_zero_where_a_is_0_or_1(rows, out_f, in_f, flags):
    ops, g, a, w, _, gz, _, _ = _backward(rows, out_f, in_f, flags)
    want = g.double() * a.double() * (1.0 - a.double())
    err = (gz.double() - want).abs()
    ok = want != 0
    print("rows %d out %d in %d flags %d: max |gz - g a (1 - a)| / |g a (1 - a)| = %.2f ULP" % (rows, out_f, in_f, flags, float((err[ok] / want[ok].abs()).max()) / ULP))
    assert bool((err <= 2.5 * ULP * want.abs()).all())
    ends = (a == 0) | (a == 1)
    assert int(ends.sum()) > 100 and bool((a == 0).any()) and bool((a == 1).any()) and bool((gz[ends] == 0).all()) and bool((gz[~ends] != 0).all())
    # within the engine's self-check bar of aten.sigmoid_backward
    assert bool(((gz - torch.ops.aten.sigmoid_backward(g, a)).abs() <= 1.5 * ULP * g.abs()).all())


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_a_nan_or_an_infinite_g_stays_in_its_element_of_gz_and_its_row_of_dx(rows, out_f, in_f, flags):
    ops, g, a, w, _, gz, _, dx = _backward(rows, out_f, in_f, flags)
    a2 = _outputs(rows, out_f, tc.case_seed(rows, in_f, out_f) + 3, True).to(ops.device)
    g2 = g.clone()
    g2[7, 3], g2[9, 1], a2[9, 1] = float("nan"), float("inf"), 0.0          # g = inf where s = 0: NaN, as in aten.sigmoid_backward
    nan = torch.isnan(a2) | torch.isnan(g2)
    nan[9, 1] = True
    assert int(nan.sum()) > 4
    gz2, dx2 = ops.linear_bwd(g2, a2, w, flags=flags, act="sigmoid")
    assert bool(torch.isnan(gz2[nan]).all()) and not bool(torch.isnan(gz2[~nan]).any())
    assert bool(torch.isnan(torch.ops.aten.sigmoid_backward(g2, a2)[9, 1]))
    want = g2.double() * a2.double() * (1.0 - a2.double())
    assert bool(((gz2.double() - want).abs()[~nan] <= 2.5 * ULP * want.abs()[~nan]).all())
    rows_nan = nan.any(1)
    assert bool(torch.isnan(dx2[rows_nan]).all()) and not bool(rows_nan.all())
    # a clean row's dx depends on that row alone: the bits of the launch in which only those rows' a and g are used
    clean = ~rows_nan
    a3, g3 = a2.clone(), g2.clone()
    a3[rows_nan], g3[rows_nan] = 0.5, 1.0
    gz3, dx3 = ops.linear_bwd(g3, a3, w, flags=flags, act="sigmoid")
    assert torch.equal(dx2[clean].view(torch.int32), dx3[clean].view(torch.int32)) and torch.equal(gz2[clean].view(torch.int32), gz3[clean].view(torch.int32))


def test_gz_has_the_same_bits_in_every_form():
    ops, g, a, w, _, gz, _, dx = _backward(256, 64, 128, 0)
    _, g1, a1, w1, _, gz_plain, _, dx_plain = _backward(256, 64, 128, PLAIN)
    assert torch.equal(g, g1) and torch.equal(a, a1) and torch.equal(w, w1)
    assert torch.equal(gz.view(torch.int32), gz_plain.view(torch.int32)) and torch.equal(dx.view(torch.int32), dx_plain.view(torch.int32))
    # the ragged body: 300 rows whose first 256 are these
    g300 = torch.cat([g, _randn(44, 64, 98).to(ops.device)])
    a300 = torch.cat([a, torch.sigmoid(_randn(44, 64, 97)).to(ops.device)])
    gz300, dx300 = ops.linear_bwd(g300, a300, w, act="sigmoid")
    assert torch.equal(gz300[:256].view(torch.int32), gz.view(torch.int32)) and torch.equal(dx300[:256].view(torch.int32), dx.view(torch.int32))


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
    ops.linear_bwd(g, a, w, gz2, dx2, flags=flags, act="sigmoid")
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


@pytest.mark.parametrize("flags", [0, PLAIN])
def test_refused_calls_return_nonzero_and_leave_the_outputs_untouched(flags):
    from pnode_amd import _lib
    from pnode_amd._lib import PnError
    ops = _ops()
    SIG = _lib.PN_ACT_SIGMOID
    rows, out_f, in_f = 256, 64, 128
    g = torch.full((rows, out_f), 8.0, device=ops.device)
    a = torch.full((rows, out_f), 0.5, device=ops.device)
    w = torch.full((out_f, in_f), 5.0, device=ops.device)
    gbuf, gz = tc.guarded(rows, out_f, ops.device)
    dbuf, dx = tc.guarded(rows, in_f, ops.device)
    xbuf, xy = tc.guarded(rows, in_f, ops.device)             # a forward output: y of x = g (256 x 64) and w^T (128 x 64)
    wt = w.t().contiguous()

    def untouched():
        torch.cuda.synchronize()
        words = (gbuf.view(torch.int32), dbuf.view(torch.int32), xbuf.view(torch.int32))
        return all(bool((v == tc.SENTINEL).all()) for v in words) and bool((g == 8.0).all()) and bool((a == 0.5).all()) and bool((w == 5.0).all())

    def last():
        return ops.lib.pn_last_error().decode()

    def fwd(act, y, x=g, rows_=rows, in_=out_f):
        return ops.lib.pn_linear_fwd_form(ops.stream(), ops.code, rows_, in_f, in_, x.data_ptr() if isinstance(x, torch.Tensor) else x,
                                          wt.data_ptr(), None, act, y.data_ptr() if isinstance(y, torch.Tensor) else y, flags)

    for act in (3, 7):
        assert _act(ops, g, a, w, act, gz, dx, flags) != 0 and "act is PN_ACT_TANH or PN_ACT_RELU" in last() and "pn_linear_dx" in last() and untouched()
        assert fwd(act, xy) != 0 and "pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU" in last() and untouched()
    assert _act(ops, g, a, w, SIG, gz, dx, flags | 2) != 0 and "pn_linear_bwd_act: unknown flag" in last() and untouched()
    # gz is g; dx is gz (256 x 64 x 64: the two have one shape); y is x
    assert _act(ops, g, a, w, SIG, g, dx, flags) != 0 and "gz must not alias" in last() and untouched()
    w64 = torch.full((64, 64), 5.0, device=ops.device)
    assert _act(ops, g, a, w64, SIG, gz, gz, flags) != 0 and "dx must not alias" in last() and untouched()
    assert _act(ops, g, a, w64, SIG, gz, gz.data_ptr() + 4 * rows * 64 - 16, flags) != 0 and "dx must not alias" in last() and untouched()
    assert fwd(SIG, g) != 0 and "y must not alias" in last() and untouched()
    # a pointer off 16 bytes, and a null one: each operand in turn
    for k in range(5):
        for bad in (lambda v: v.data_ptr() + 4, lambda v: None):
            args = [g, a, w, gz, dx]
            args[k] = bad(args[k])
            assert _act(ops, args[0], args[1], args[2], SIG, args[3], args[4], flags, rows, out_f, in_f) != 0
            assert "16-byte aligned" in last() or "null operand" in last()
    assert fwd(SIG, xy.data_ptr() + 4) != 0 and "16-byte aligned" in last() and fwd(SIG, xy, x=None) != 0 and "null operand" in last()
    assert untouched()
    # shapes outside pn_linear_bwd_supported / pn_linear_fwd_supported: 255 and 128 rows, K = 80 and 48, 100 columns; an fp64 state
    for r, o, i in ((255, out_f, in_f), (128, out_f, in_f), (rows, 80, in_f), (rows, 48, in_f), (rows, out_f, 100)):
        assert not ops.linear_bwd_supported(r, o, i)
        assert _act(ops, g, a, w, SIG, gz, dx, flags, r, o, i) != 0 and "unsupported dtype or shape" in last()
    for r, k in ((255, out_f), (rows, 80)):
        assert not ops.linear_fwd_supported(r, in_f, k)
        assert fwd(SIG, xy, rows_=r, in_=k) != 0 and "unsupported dtype or shape" in last()
    assert ops.lib.pn_linear_bwd_act(ops.stream(), 1, rows, out_f, in_f, g.data_ptr(), a.data_ptr(), w.data_ptr(), SIG, gz.data_ptr(),
                                     dx.data_ptr(), flags) != 0 and "unsupported dtype or shape" in last()
    assert untouched()
    # the backend refuses an activation it does not know, by name, before any launch
    with pytest.raises(PnError, match="tanh or relu or sigmoid"):
        ops.linear_bwd(g, a, w, gz, dx, flags=flags, act="identity")
    with pytest.raises(PnError, match="identity, tanh or relu or sigmoid"):
        ops.linear_fwd(g, wt, None, False, flags=flags, act="gelu")
    assert untouched()
    # and the same operands, not aliased, go through: a = 1/2 everywhere, so gz is g / 4 = 2 and dx is 64 * 2 * 5, all exact; the forward
    # of x = 8, w = 5 over K = 64 is z = 2560: exactly 1
    assert _act(ops, g, a, w, SIG, gz, dx, flags) == 0 and fwd(SIG, xy) == 0
    torch.cuda.synchronize()
    assert bool((gz == 2.0).all()) and bool((dx == out_f * 2.0 * 5.0).all()) and bool((xy == 1.0).all())
    assert tc.guards_untouched(gbuf, rows) and tc.guards_untouched(dbuf, rows) and tc.guards_untouched(xbuf, rows)
