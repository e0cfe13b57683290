"""-m gpu: the GELU forms of pn_linear_fwd (PN_ACT_GELU), pn_linear_fwd_pre (the pre-activation beside y) and pn_linear_bwd_act
(csrc/pn_linear.hip), through HipVecOps.

Shapes (rows, out_f, in_f): the cases of tests/test_gpu_linear_sigmoid.py.  Forward (K = in_f): 256 x 128 x 64 aligned, two slabs:
pipelined, and the same with PN_LINEAR_FORM_PLAIN; 256 x 128 x 96 three slabs -- an odd number: the plain loop; 300 x 192 x 64 ragged in
rows and columns; each with and without a bias.  Backward (K = out_f, columns = in_f): 256 x 64 x 128, the same plain, 256 x 96 x 128,
300 x 64 x 192.

What is exact is asserted bit for bit: z of pn_linear_fwd_pre is the identity kernel's y, y of pn_linear_fwd_pre the y-only form's, y and
gz the same in every form, dx the bits of pn_linear_dx fed gz, y == z for z >= 6 and y == -0 for z <= -6.  What is not -- the device
library's erff and expf have no bound stated in this repository -- is measured against float64 and held to MARGIN = 2 (the margin of
tests/test_gpu_linear_fwd.py) times the error of the stock fp32 operation on the SAME operands in the SAME measure, per case:
  forward   max |y - gelu64(z)| over the case, z the identity kernel's result, against F.gelu(z) in fp32;
  backward  max |gz - g d64(z)| / |g| -- absolute in d = cdf + z pdf, which crosses zero near z = -0.7518 -- against
            aten.gelu_backward(g, z) in fp32;
  random operands end to end: |y - y64| / (sum |x w| + |b|) against F.gelu(F.linear) on the same operands.
Measured on MI355X over the cases: forward max |y - gelu64(z)| 3.98 to 6.73 ULP (1.79 to 1.88 ULP relative to max(1, |z|)) -- F.gelu's own
figures on the same z, digit for digit (it evidently runs the same erff); exact operands 6.43 ULP on both sides; backward 2.63 to 2.66
ULP against aten.gelu_backward's 2.63 to 2.65; random operands end to end 1.195e-7 to 1.459e-7 against the library pair's 1.911e-7 to
2.693e-7, worst ratio 0.63.  y == z from z >= 6 and y == -0 from z <= -6 hold as written.  Below z = -6 the derivative is not 0 but
z pdf (6 pdf(6) = 3.6e-8): gz is that small, not zero, until expf underflows."""
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
UP_ROW, DOWN_ROW = 5, 6               # rows of the exact operands driven to z >= 6 and to z <= -6
MINUS_ZERO = -2 ** 31                 # the bits of -0.0 as an int32


def _ops():
    from pnode_amd import _lib, _linearfwd
    from pnode_amd._vecops import HipVecOps
    assert _lib.PN_LINEAR_FORM_PLAIN == PLAIN and _linearfwd.CHECK_TOL == CHECK_TOL and HipVecOps.linear_gelu is True
    assert _lib.PN_ACT_GELU == 8
    return HipVecOps(require_gpu(), torch.float32, 300 * 192)


def _randn(rows, cols, seed):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


def _randint(lo, hi, rows, cols, seed):
    return torch.randint(lo, hi + 1, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


def _gelu64(z):
    z = z.double()
    return 0.5 * z * (1.0 + torch.erf(z * 0.5 ** 0.5))


def _d64(z):
    """GELU's derivative in float64: Phi(z) + z phi(z)."""
    z = z.double()
    return 0.5 * (1.0 + torch.erf(z * 0.5 ** 0.5)) + z * torch.exp(-0.5 * z * z) * (2.0 * torch.pi) ** -0.5


def _bits(v):
    return v.contiguous().view(torch.int32)


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


def _launches(ops, x, w, b, flags):
    """(y and z of pn_linear_fwd_pre -- inside guards --, y of the y-only form, y of the identity)."""
    rows, out_f = x.shape[0], w.shape[0]
    ybuf, y = tc.guarded(rows, out_f, ops.device)
    zbuf, z = tc.guarded(rows, out_f, ops.device)
    out = ops.linear_act_fwd(x, w, b, "gelu", y, z, flags=flags)
    torch.cuda.synchronize()
    assert out is y
    y_only = ops.linear_act_fwd(x, w, b, "gelu", flags=flags)
    ident = ops.linear_fwd(x, w, b, False, flags=flags)
    assert ops.linear_fwd_supported(rows, out_f, x.shape[1]) and y_only.shape == (rows, out_f) and y_only.dtype == torch.float32
    return ybuf, y, zbuf, z, y_only, ident


def _forward(rows, out_f, in_f, flags, bias):
    """Operands N(0, 1), w scaled by in_f^-1/2 (z of a few units on either side of 0), and the GELU and identity results."""
    key = (rows, out_f, in_f, flags, bias)
    if key not in _FWD:
        ops = _ops()
        seed = tc.case_seed(rows, out_f, in_f)
        x = _randn(rows, in_f, seed).to(ops.device)
        w = (_randn(out_f, in_f, seed + 17) * in_f ** -0.5).to(ops.device)
        b = _randn(1, out_f, seed + 5).view(-1).to(ops.device) if bias else None
        _FWD[key] = (ops, x, w, b) + _launches(ops, x, w, b, flags)
    return _FWD[key]


def _exact(rows, out_f, in_f, flags, bias):
    """Small-integer operands: x in quarters of -4 .. 4, w in quarters of -2 .. 2, b in quarters of -8 .. 8 -- every product a multiple of
    1/16 below 1, every sum exact in fp32 in any order and in the split.  Row UP_ROW of x is +4 and row DOWN_ROW -8 against column 0
    and 1 of w set to +1/4 throughout: z = in_f + b >= 62 there, z = -2 in_f + b <= -126."""
    key = ("exact", rows, out_f, in_f, flags, bias)
    if key not in _FWD:
        ops = _ops()
        seed = tc.case_seed(rows, out_f, in_f)
        x, w = _randint(-4, 4, rows, in_f, seed) / 4, _randint(-2, 2, out_f, in_f, seed + 17) / 4
        x[UP_ROW], x[DOWN_ROW] = 4.0, -8.0
        w[0], w[1] = 0.25, 0.25
        b = _randint(-8, 8, 1, out_f, seed + 5).view(-1) / 4 if bias else None
        x, w, b = x.to(ops.device), w.to(ops.device), None if b is None else b.to(ops.device)
        _FWD[key] = (ops, x, w, b) + _launches(ops, x, w, b, flags)
    return _FWD[key]


def _fwd_cases():
    return pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)


@pytest.mark.parametrize("bias", [True, False])
@_fwd_cases()
def test_z_is_the_identity_kernels_y_and_y_is_the_y_only_forms_bit_for_bit(rows, out_f, in_f, flags, bias):
    for make in (_forward, _exact):
        ops, x, w, b, _, y, _, z, y_only, ident = make(rows, out_f, in_f, flags, bias)
        assert torch.equal(_bits(z), _bits(ident)) and torch.equal(_bits(y), _bits(y_only))
    # z is written for any act, and leaves y what it is without z: the identity (z == y), tanh, relu, sigmoid
    ops, x, w, b, _, _, _, z, _, ident = _forward(rows, out_f, in_f, flags, bias)
    for act in ("identity", "tanh", "relu", "sigmoid"):
        z2 = torch.full_like(ident, float("nan"))
        y2 = ops.linear_act_fwd(x, w, b, act, z=z2, flags=flags)
        assert torch.equal(_bits(z2), _bits(ident)) and torch.equal(_bits(y2), _bits(ops.linear_fwd(x, w, b, False, flags=flags, act=act)))


@pytest.mark.parametrize("bias", [True, False])
@_fwd_cases()
def test_gelu_forward_is_gelu_of_the_identity_forward_within_twice_f_gelus_own_error(rows, out_f, in_f, flags, bias):
    ops, x, w, b, _, y, _, z, _, ident = _forward(rows, out_f, in_f, flags, bias)
    assert bool(torch.isfinite(ident).all()) and bool((ident < -1).any()) and bool((ident > 1).any()) and float(ident.abs().max()) < 15.0
    ref = _gelu64(ident)
    own, lib = (y.double() - ref).abs(), (F.gelu(ident).double() - ref).abs()
    print("rows %d out %d in %d flags %d bias %s: max |y - gelu64(z)| = %.2f ULP, F.gelu %.2f ULP; over max(1, |z|): %.2f and %.2f ULP"
          % (rows, out_f, in_f, flags, bias, float(own.max()) / ULP, float(lib.max()) / ULP,
             float((own / ident.double().abs().clamp(min=1)).max()) / ULP, float((lib / ident.double().abs().clamp(min=1)).max()) / ULP))
    assert float(lib.max()) > 0 and float(own.max()) <= MARGIN * float(lib.max()), (float(own.max()) / ULP, float(lib.max()) / ULP)
    # "identity" by name is what the positional flag says
    assert torch.equal(ident, ops.linear_fwd(x, w, b, True, flags=flags, act="identity"))


@pytest.mark.parametrize("bias", [True, False])
@_fwd_cases()
def test_exact_operands_against_float64(rows, out_f, in_f, flags, bias):
    ops, x, w, b, _, y, _, z, _, ident = _exact(rows, out_f, in_f, flags, bias)
    z64 = tc.forward64(x, w, b)
    zf = z64.float()
    assert torch.equal(zf.double(), z64) and torch.equal(ident, zf) and torch.equal(z, zf)   # the premise: z is exact, and both kernels give it
    ref = _gelu64(z64)
    own, lib = (y.double() - ref).abs(), (F.gelu(zf).double() - ref).abs()
    mid = zf.abs() < 6                             # (beyond: exact, the next test)
    print("rows %d out %d in %d flags %d bias %s: max |y - gelu64(z)| = %.2f ULP, F.gelu %.2f ULP"
          % (rows, out_f, in_f, flags, bias, float(own[mid].max()) / ULP, float(lib[mid].max()) / ULP))
    assert bool(mid.any()) and float(own[mid].max()) <= MARGIN * float(lib[mid].max())
    # GELU's range: never below its minimum -0.17 (at z = -0.7518), never above z's positive part by more than the bar
    assert bool((y >= -0.17).all()) and bool((y[zf > 0] > 0).all()) and bool((y[zf == 0] == 0).all())


@pytest.mark.parametrize("bias", [True, False])
@_fwd_cases()
def test_from_z_6_on_y_is_z_and_from_minus_6_down_y_is_minus_zero(rows, out_f, in_f, flags, bias):
    _, _, _, _, _, y, _, z, _, ident = _exact(rows, out_f, in_f, flags, bias)
    assert float(ident[UP_ROW, :2].min()) >= 6.0 and float(ident[DOWN_ROW, :2].max()) <= -6.0
    assert torch.equal(_bits(y[UP_ROW, :2]), _bits(ident[UP_ROW, :2])) and bool((_bits(y[DOWN_ROW, :2]) == MINUS_ZERO).all())
    # ... and wherever else the exact z is that far out
    up, down = ident >= 6.0, ident <= -6.0
    assert int(up.sum()) >= 2 and int(down.sum()) >= 2
    assert torch.equal(_bits(y[up]), _bits(ident[up])) and bool((_bits(y[down]) == MINUS_ZERO).all())


def test_random_operands_against_float64_within_twice_the_library_pairs_own_error():
    """Measured on MI355X: worst ratio own / library over the eight cases 0.63 (1.195e-7 .. 1.459e-7 against 1.911e-7 .. 2.693e-7)."""
    worst = 0.0
    for rows, out_f, in_f, flags in FWD_CASES:
        for bias in (True, False):
            ops, x, w, b, _, y, _, _, _, _ = _forward(rows, out_f, in_f, flags, bias)
            ref = _gelu64(tc.forward64(x, w, b))
            scale = x.double().abs() @ w.double().abs().t()
            if b is not None:
                scale = scale + b.double().abs()
            lib = F.gelu(F.linear(x, w, b))
            e_own = float(((y.double() - ref).abs() / scale).max())
            e_lib = float(((lib.double() - ref).abs() / scale).max())
            worst = max(worst, e_own / e_lib)
            print("rows %d out %d in %d flags %d bias %d: pn_linear_fwd_pre %.3e  library %.3e  ratio %.2f" % (rows, out_f, in_f, flags, bias, e_own, e_lib, e_own / e_lib))
            assert e_own <= MARGIN * e_lib, (rows, out_f, in_f, flags, bias, e_own, e_lib)
    print("worst ratio %.2f" % worst)


@pytest.mark.parametrize("bias", [True, False])
@_fwd_cases()
def test_a_nan_row_of_x_gives_a_nan_row_of_y_and_of_z_and_leaves_every_other_rows_bits(rows, out_f, in_f, flags, bias):
    ops, x, w, b, _, y, _, z, _, _ = _forward(rows, out_f, in_f, flags, bias)
    x2 = x.clone()
    x2[rows - 2] = float("nan")
    z2 = torch.zeros_like(z)
    y2 = ops.linear_act_fwd(x2, w, b, "gelu", z=z2, flags=flags)
    y3 = ops.linear_act_fwd(x2, w, b, "gelu", flags=flags)
    others = torch.ones(rows, dtype=torch.bool, device=ops.device)
    others[rows - 2] = False
    assert bool(torch.isnan(y2[rows - 2]).all()) and bool(torch.isnan(z2[rows - 2]).all()) and bool(torch.isnan(y3[rows - 2]).all())
    assert torch.equal(_bits(y2[others]), _bits(y[others])) and torch.equal(_bits(z2[others]), _bits(z[others]))
    assert torch.equal(_bits(y3[others]), _bits(y[others]))


@pytest.mark.parametrize("bias", [True, False])
def test_the_forward_has_the_same_bits_in_every_form(bias):
    ops, x, w, b, _, y, _, z, _, _ = _forward(256, 128, 64, 0, bias)
    _, x1, w1, b1, _, y_plain, _, z_plain, _, _ = _forward(256, 128, 64, PLAIN, bias)
    assert torch.equal(x, x1) and torch.equal(w, w1)
    assert torch.equal(_bits(y), _bits(y_plain)) and torch.equal(_bits(z), _bits(z_plain))
    # the ragged body: 300 rows whose first 256 are these -- a row of y depends on that row of x, on w and on b alone
    x300 = torch.cat([x, _randn(44, 64, 99).to(ops.device)])
    z300 = torch.zeros(300, 128, device=ops.device)
    y300 = ops.linear_act_fwd(x300, w, b, "gelu", z=z300)
    assert not tc.is_aligned(300, 128) and torch.equal(_bits(y300[:256]), _bits(y)) and torch.equal(_bits(z300[:256]), _bits(z))
    assert torch.equal(_bits(ops.linear_act_fwd(x300, w, b, "gelu")), _bits(y300))


@pytest.mark.parametrize("bias", [True, False])
@_fwd_cases()
def test_the_sentinels_around_y_and_z_stay_and_a_second_launch_gives_the_same_bits(rows, out_f, in_f, flags, bias):
    ops, x, w, b, ybuf, y, zbuf, z, _, _ = _forward(rows, out_f, in_f, flags, bias)
    assert tc.guards_untouched(ybuf, rows) and tc.guards_untouched(zbuf, rows)
    ybuf2, y2 = tc.guarded(rows, out_f, ops.device)
    zbuf2, z2 = tc.guarded(rows, out_f, ops.device)
    ops.linear_act_fwd(x, w, b, "gelu", y2, z2, flags=flags)
    buf3, y3 = tc.guarded(rows, out_f, ops.device)
    ops.linear_act_fwd(x, w, b, "gelu", y3, flags=flags)
    torch.cuda.synchronize()
    assert tc.guards_untouched(ybuf2, rows) and tc.guards_untouched(zbuf2, rows) and tc.guards_untouched(buf3, rows)
    assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(z2), _bits(z)) and torch.equal(_bits(y3), _bits(y))


# ------------------------------------------------------------------------------------------------------------------------ backward
_BWD = {}


def _pre_activations(rows, k, seed, nans):
    """The pair's pre-activation as the kernel may meet it: N(0, 4), exact zeros, the zero of the derivative, values beyond +-6 and,
    with `nans`, a few NaNs."""
    z = 2.0 * _randn(rows, k, seed)
    pick = torch.randint(0, 16, (rows, k), generator=torch.Generator().manual_seed(seed + 1))
    z[pick == 0] = 0.0
    z[pick == 1] = -0.7518
    z[pick == 2] = 7.5
    z[pick == 3] = -7.5
    if nans:
        z[16:24][pick[16:24] == 4] = float("nan")                 # (eight rows of them; the other rows stay clean)
        z[0, 0], z[rows - 1, k - 1] = float("nan"), float("nan")
    z[1, 1], z[2, 2] = 0.0, -0.7518
    return z


def _backward(rows, out_f, in_f, flags):
    key = (rows, out_f, in_f, flags)
    if key not in _BWD:
        ops = _ops()
        seed = tc.case_seed(rows, in_f, out_f)
        g = _randn(rows, out_f, seed)
        g[g.abs() < 1e-3] = 1e-3                   # (the normal range, well away from a product that underflows)
        g = g.to(ops.device)
        w = (_randn(out_f, in_f, seed + 17) * out_f ** -0.5).to(ops.device)
        z = _pre_activations(rows, out_f, seed + 3, False).to(ops.device)
        gbuf, gz = tc.guarded(rows, out_f, ops.device)
        dbuf, dx = tc.guarded(rows, in_f, ops.device)
        out = ops.linear_bwd(g, z, w, gz, dx, flags=flags, act="gelu")
        torch.cuda.synchronize()
        assert out[0] is gz and out[1] is dx and ops.linear_bwd_supported(rows, out_f, in_f)
        _BWD[key] = (ops, g, z, w, gbuf, gz, dbuf, dx)
    return _BWD[key]


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_gz_is_g_times_gelus_derivative_within_twice_gelu_backwards_own_error(rows, out_f, in_f, flags):
    ops, g, z, w, _, gz, _, _ = _backward(rows, out_f, in_f, flags)
    want = g.double() * _d64(z)
    aten = torch.ops.aten.gelu_backward(g, z, approximate="none")
    own = (gz.double() - want).abs() / g.double().abs()
    lib = (aten.double() - want).abs() / g.double().abs()
    print("rows %d out %d in %d flags %d: max |gz - g d64(z)| / |g| = %.2f ULP, aten.gelu_backward %.2f ULP"
          % (rows, out_f, in_f, flags, float(own.max()) / ULP, float(lib.max()) / ULP))
    assert float(lib.max()) > 0 and float(own.max()) <= MARGIN * float(lib.max()), (float(own.max()) / ULP, float(lib.max()) / ULP)
    # d is exactly 1 from z = 6 on: gz is g; from -6 down cdf is 0 and d = z pdf, below 4e-8 in size (6 pdf(6) = 3.6e-8)
    assert int((z >= 6).sum()) > 100 and int((z <= -6).sum()) > 100 and int((z == 0).sum()) > 100
    assert torch.equal(_bits(gz[z >= 6]), _bits(g[z >= 6])) and bool((gz[z <= -6].abs() <= 4e-8 * g[z <= -6].abs()).all())
    assert torch.equal(gz[z == 0], 0.5 * g[z == 0])                          # cdf(0) = 1/2, z pdf = 0: exact
    # within the engine's self-check bar of aten.gelu_backward
    assert bool(((gz - aten).abs() <= 32.0 * ULP * g.abs()).all())


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_a_nan_or_an_infinite_g_stays_in_its_element_of_gz_and_its_row_of_dx(rows, out_f, in_f, flags):
    ops, g, z, w, _, gz, _, dx = _backward(rows, out_f, in_f, flags)
    z2 = _pre_activations(rows, out_f, tc.case_seed(rows, in_f, out_f) + 3, True).to(ops.device)
    g2 = g.clone()
    g2[7, 3], g2[9, 1], z2[9, 1] = float("nan"), float("inf"), -20.0        # g = inf where d = 0 (expf(-200) is 0): NaN, as in aten.gelu_backward
    g2[11, 2], z2[11, 2] = float("inf"), 1.0                                # g = inf where d > 0: inf in gz, NaN in its row of dx (inf - inf in the split)
    nan = torch.isnan(z2) | torch.isnan(g2)
    nan[9, 1] = True
    assert int(nan.sum()) > 4
    gz2, dx2 = ops.linear_bwd(g2, z2, w, flags=flags, act="gelu")
    assert bool(torch.isnan(gz2[nan]).all()) and not bool(torch.isnan(gz2[~nan]).any())
    assert bool(torch.isnan(torch.ops.aten.gelu_backward(g2, z2, approximate="none")[9, 1])) and float(gz2[11, 2]) == float("inf")
    rows_bad = nan.any(1)
    rows_bad[11] = True
    assert bool(torch.isnan(dx2[rows_bad]).all()) and not bool(rows_bad.all())
    # a clean row's gz and dx depend on that row alone: the bits of the launch in which only those rows' z and g are used
    clean = ~rows_bad
    z3, g3 = z2.clone(), g2.clone()
    z3[rows_bad], g3[rows_bad] = 0.5, 1.0
    gz3, dx3 = ops.linear_bwd(g3, z3, w, flags=flags, act="gelu")
    assert not bool(torch.isnan(dx3).any())
    assert torch.equal(_bits(dx2[clean]), _bits(dx3[clean])) and torch.equal(_bits(gz2[clean]), _bits(gz3[clean]))


def test_gz_has_the_same_bits_in_every_form():
    ops, g, z, w, _, gz, _, dx = _backward(256, 64, 128, 0)
    _, g1, z1, w1, _, gz_plain, _, dx_plain = _backward(256, 64, 128, PLAIN)
    assert torch.equal(g, g1) and torch.equal(z, z1) and torch.equal(w, w1)
    assert torch.equal(_bits(gz), _bits(gz_plain)) and torch.equal(_bits(dx), _bits(dx_plain))
    # the ragged body: 300 rows whose first 256 are these
    g300 = torch.cat([g, _randn(44, 64, 98).to(ops.device)])
    z300 = torch.cat([z, _randn(44, 64, 97).to(ops.device)])
    gz300, dx300 = ops.linear_bwd(g300, z300, w, act="gelu")
    assert torch.equal(_bits(gz300[:256]), _bits(gz)) and torch.equal(_bits(dx300[:256]), _bits(dx))


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_dx_has_the_bits_of_pn_linear_dx_fed_gz(rows, out_f, in_f, flags):
    ops, g, z, w, _, gz, _, dx = _backward(rows, out_f, in_f, flags)
    assert not bool(torch.isnan(z).any()) and not bool(torch.isnan(g).any())
    want = ops.linear_dx(gz.contiguous(), w, flags=flags)
    assert dx.shape == (rows, in_f) and torch.equal(_bits(dx), _bits(want)), int((dx != want).sum())
    # ... and is as far from float64 as the engine's self-check allows at most
    ref = gz.double() @ w.double()
    scale = gz.double().abs() @ w.double().abs()
    assert bool(((dx.double() - ref).abs() <= CHECK_TOL * scale).all())


@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_the_sentinels_around_gz_and_dx_stay_and_a_second_launch_gives_the_same_bits(rows, out_f, in_f, flags):
    ops, g, z, w, gbuf, gz, dbuf, dx = _backward(rows, out_f, in_f, flags)
    assert tc.guards_untouched(gbuf, rows) and tc.guards_untouched(dbuf, rows)
    gbuf2, gz2 = tc.guarded(rows, out_f, ops.device)
    dbuf2, dx2 = tc.guarded(rows, in_f, ops.device)
    ops.linear_bwd(g, z, w, gz2, dx2, flags=flags, act="gelu")
    torch.cuda.synchronize()
    assert tc.guards_untouched(gbuf2, rows) and tc.guards_untouched(dbuf2, rows)
    assert torch.equal(_bits(gz2), _bits(gz)) and torch.equal(_bits(dx2), _bits(dx))


# ------------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("flags", [0, PLAIN])
def test_refused_calls_return_nonzero_and_leave_the_outputs_untouched(flags):
    from pnode_amd import _lib
    from pnode_amd._lib import PnError
    ops = _ops()
    GELU = _lib.PN_ACT_GELU
    rows, out_f, in_f = 256, 64, 128
    g = torch.full((rows, out_f), 8.0, device=ops.device)
    a = torch.full((rows, out_f), 0.0, device=ops.device)
    w = torch.full((out_f, in_f), 5.0, device=ops.device)
    gbuf, gz = tc.guarded(rows, out_f, ops.device)
    dbuf, dx = tc.guarded(rows, in_f, ops.device)
    xbuf, xy = tc.guarded(rows, in_f, ops.device)             # the forward outputs: y and z of x = g (256 x 64) and w^T (128 x 64)
    zbuf, xz = tc.guarded(rows, in_f, ops.device)
    wt = w.t().contiguous()

    def ptr(v):
        return v.data_ptr() if isinstance(v, torch.Tensor) else v

    def untouched():
        torch.cuda.synchronize()
        words = (gbuf.view(torch.int32), dbuf.view(torch.int32), xbuf.view(torch.int32), zbuf.view(torch.int32))
        return all(bool((v == tc.SENTINEL).all()) for v in words) and bool((g == 8.0).all()) and bool((a == 0.0).all()) and bool((w == 5.0).all())

    def last():
        return ops.lib.pn_last_error().decode()

    def bwd(act, gz_, dx_, g_=g, a_=a, w_=w, flags_=flags, rows_=rows, out_=out_f, in_=in_f, dtype=None):
        return ops.lib.pn_linear_bwd_act(ops.stream(), ops.code if dtype is None else dtype, rows_, out_, in_, ptr(g_), ptr(a_), ptr(w_), act,
                                         ptr(gz_), ptr(dx_), flags_)

    def pre(act, y, z, x=g, flags_=flags, rows_=rows, k=out_f, dtype=None):
        return ops.lib.pn_linear_fwd_pre(ops.stream(), ops.code if dtype is None else dtype, rows_, in_f, k, ptr(x), wt.data_ptr(), None, act,
                                         ptr(y), ptr(z), flags_)

    for act in (3, 5, 7, -1):
        assert bwd(act, gz, dx) != 0 and "act is PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU" in last() and untouched()
        assert pre(act, xy, xz) != 0 and "pn_linear_fwd: act is PN_ACT_IDENTITY, PN_ACT_TANH or PN_ACT_RELU or PN_ACT_SIGMOID or PN_ACT_GELU" in last()
    assert bwd(GELU, gz, dx, flags_=flags | 2) != 0 and "pn_linear_bwd_act: unknown flag" in last() and untouched()
    assert pre(GELU, xy, xz, flags_=flags | 2) != 0 and "pn_linear_fwd_pre: unknown flag" in last() and untouched()
    # aliases: gz is g; y is x; z is y, x, w; z is null or off 16 bytes
    assert bwd(GELU, g, dx) != 0 and "gz must not alias" in last() and untouched()
    assert pre(GELU, g, xz) != 0 and "y must not alias" in last() and untouched()
    for alias in (xy, g, wt, xy.data_ptr() + 4 * rows * in_f - 16):
        assert pre(GELU, xy, alias) != 0 and "z must not alias y, x, w or b" in last() and untouched()
    assert pre(GELU, xy, None) != 0 and "z is null" in last() and pre(GELU, xy, xz.data_ptr() + 4) != 0 and "z must be 16-byte aligned" in last()
    assert pre(GELU, xy.data_ptr() + 4, xz) != 0 and "16-byte aligned" in last() and pre(GELU, xy, xz, x=None) != 0 and "null operand" in last()
    assert untouched()
    # shapes outside pn_linear_fwd_supported / pn_linear_bwd_supported; an fp64 state
    for r, k in ((255, out_f), (128, out_f), (rows, 80)):
        assert not ops.linear_fwd_supported(r, in_f, k)
        assert pre(GELU, xy, xz, rows_=r, k=k) != 0 and "unsupported dtype or shape" in last()
    for r, o, i in ((255, out_f, in_f), (128, out_f, in_f), (rows, 80, in_f), (rows, out_f, 100)):
        assert not ops.linear_bwd_supported(r, o, i)
        assert bwd(GELU, gz, dx, rows_=r, out_=o, in_=i) != 0 and "unsupported dtype or shape" in last()
    assert pre(GELU, xy, xz, dtype=1) != 0 and "unsupported dtype or shape" in last()
    assert bwd(GELU, gz, dx, dtype=1) != 0 and "unsupported dtype or shape" in last()
    assert untouched()
    # the backend refuses a name it does not know before any launch; linear_fwd keeps refusing "gelu": its door is linear_act_fwd
    with pytest.raises(PnError, match="tanh or relu or sigmoid or gelu"):
        ops.linear_bwd(g, a, w, gz, dx, flags=flags, act="identity")
    with pytest.raises(PnError, match="identity, tanh or relu or sigmoid or gelu"):
        ops.linear_act_fwd(g, wt, None, "silu", flags=flags)
    with pytest.raises(PnError, match="identity, tanh or relu or sigmoid"):
        ops.linear_fwd(g, wt, None, False, flags=flags, act="gelu")
    assert untouched()
    # and the same operands, not aliased, go through: z = 0 everywhere, so gz is g / 2 = 4 and dx is 64 * 4 * 5, all exact; the forward
    # of x = 8, w = 5 over K = 64 is z = 2560, and y is z
    assert bwd(GELU, gz, dx) == 0 and pre(GELU, xy, xz) == 0
    torch.cuda.synchronize()
    assert bool((gz == 4.0).all()) and bool((dx == out_f * 4.0 * 5.0).all()) and bool((xy == 2560.0).all()) and bool((xz == 2560.0).all())
    assert all(tc.guards_untouched(buf, rows) for buf in (gbuf, dbuf, xbuf, zbuf))
