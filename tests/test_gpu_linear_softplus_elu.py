"""-m gpu: the Softplus and ELU forms of pn_linear_fwd / pn_linear_fwd_pre (PN_ACT_SOFTPLUS, PN_ACT_ELU) and pn_linear_bwd_act
(csrc/pn_linear.hip), through HipVecOps.

Shapes (rows, out_f, in_f): the cases of tests/test_gpu_linear_sigmoid.py, the smallest that reach the pipelined, plain and ragged
instantiations; each with and without a bias.

DERIVED bars (ULP = 2^-24): ELU forward y == z bit for bit where z > 0; ELU g_z == g bit for bit where a > 0, within 1.5 ULP |g| of the
float64 g (a + 1) where a <= 0 (one rounded add of magnitude <= 1, one rounded product); Softplus g_z == g bit for bit where a >= 18;
saturation on the exact operands: Softplus y == z for z >= 62 and y == +0 for z <= -126, ELU y == z and y == -1; dx bitwise
linear_dx(g_z, w); y, g_z and dx the same bits in the three forms and with or without z; a NaN row of x gives a NaN row and leaves every
other row's bits; a NaN or +-inf in g stays in its element of g_z and its row of dx.

MEASURED bars: the device library states no bound for log1pf and expm1f.  On a grid of pre-activations over [-104, 89] plus 0 and the
thresholds (z taken from pn_linear_fwd_pre), the kernel's y against float64 of its own z, relative to max(|y|, 2^-126), beside what
F.softplus / F.elu give on the same fp32 z; for Softplus' g_z, against float64 g (1 - e^-a) relative to |g|, beside
g * (-torch.expm1(-a)).  The bar is the library's measured worst plus one ULP (the same two functions, another library build), capped
at 4 ULP.  Measured on MI355X (LIB_* below are the library's figures, the kernel's beside them):
    Softplus forward  library 1.999 ULP, kernel 1.999 ULP: the bar is 2.999
    ELU forward       library 1.231 ULP, kernel 1.231 ULP: the bar is 2.231
    Softplus g_z      library 1.428 ULP, kernel 1.428 ULP: the bar is 2.428
(the kernel's figures are the library's digit for digit: the same device functions).  Off the grid, on the random operands of the eight
cases, the forward's worst is 2.16 ULP (Softplus) and 1.39 ULP (ELU), g_z's 1.46 and 1.40.

Random operands against float64 in the pairs' measure |y - y64| / (sum |x w| + |b|): at most MARGIN = 2 times the stock pair's own error on
the same operands (the bar of tests/test_gpu_linear_sigmoid.py)."""
import pytest
import torch
import torch.nn.functional as F

import _linear_tile_cases as tc
from conftest import require_gpu

pytestmark = pytest.mark.gpu

PLAIN = 1                             # PN_LINEAR_FORM_PLAIN
ULP = 2.0 ** -24
TINY = 2.0 ** -126
MARGIN = 2.0
CHECK_TOL = 1e-6
CAP = 4.0                             # ULP: a condition on both measured bars
# measured on MI355X on the grid below, in ULP: (the library's worst, the kernel's worst)
LIB_SOFTPLUS_Y, KERNEL_SOFTPLUS_Y = 1.999, 1.999
LIB_ELU_Y, KERNEL_ELU_Y = 1.231, 1.231
LIB_SOFTPLUS_GZ, KERNEL_SOFTPLUS_GZ = 1.428, 1.428
BAR_Y = {"softplus": LIB_SOFTPLUS_Y + 1.0, "elu": LIB_ELU_Y + 1.0}
BAR_SOFTPLUS_GZ = LIB_SOFTPLUS_GZ + 1.0
ACTS = ["softplus", "elu"]
FWD_CASES = [(256, 128, 64, 0), (256, 128, 64, PLAIN), (256, 128, 96, 0), (300, 192, 64, 0)]
BWD_CASES = [(256, 64, 128, 0), (256, 64, 128, PLAIN), (256, 96, 128, 0), (300, 64, 192, 0)]
HIGH_ROW, LOW_ROW = 5, 6              # rows of the exact operands driven to z >= 62 and to z <= -126


def _ops():
    from pnode_amd import _lib, _linearfwd
    from pnode_amd._vecops import HipVecOps
    assert _lib.PN_LINEAR_FORM_PLAIN == PLAIN and _linearfwd.CHECK_TOL == CHECK_TOL
    assert HipVecOps.linear_softplus is True and HipVecOps.linear_elu is True and (_lib.PN_ACT_SOFTPLUS, _lib.PN_ACT_ELU) == (16, 32)
    return HipVecOps(require_gpu(), torch.float32, 300 * 192)


def _randn(rows, cols, seed):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


def _randint(lo, hi, rows, cols, seed):
    return torch.randint(lo, hi + 1, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


def _y64(act, z64):
    """float64 of the activation, by the stable expressions (no threshold: log1p(e^z) - z is far below the spacing of z there)."""
    if act == "softplus":
        return torch.clamp(z64, min=0) + torch.log1p(torch.exp(-z64.abs()))
    return torch.where(z64 > 0, z64, torch.expm1(z64))


def _stock(act, z):
    return F.softplus(z) if act == "softplus" else F.elu(z)


def _gz64(act, g, a):
    g, a = g.double(), a.double()
    return g * (-torch.expm1(-a)) if act == "softplus" else torch.where(a > 0, g, g * (a + 1.0))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_the_bars_are_the_librarys_figure_plus_one_ulp_and_under_the_caps():
    assert BAR_Y["softplus"] == LIB_SOFTPLUS_Y + 1.0 <= CAP and BAR_Y["elu"] == LIB_ELU_Y + 1.0 <= CAP
    assert BAR_SOFTPLUS_GZ == LIB_SOFTPLUS_GZ + 1.0 <= CAP


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


# ---------------------------------------------------------------------------------------------------------------- the measured bars
_GRID = {}
GRID_ROWS, GRID_COLS, EXTRA_ROWS = 1024, 128, 64


def _grid(act):
    """z = base[r] + delta[c] over [-104, 89.2] in steps of about 1.5e-3, formed by the kernel itself (x = (base, 1, 0, ...), w = (1,
    delta, 0, ...)); the rows behind them are +0 and the thresholds: 20, the float above 20, +-1e-4 around 0, and 18.  y and z from
    pn_linear_fwd_pre, y alone from pn_linear_fwd."""
    if act not in _GRID:
        ops = _ops()
        x = torch.zeros(GRID_ROWS + EXTRA_ROWS, 64)
        w = torch.zeros(GRID_COLS, 64)
        x[:GRID_ROWS, 0] = torch.linspace(-104.0, 89.0, GRID_ROWS)
        x[:GRID_ROWS, 1] = 1.0
        w[:, 0] = 1.0
        w[:, 1] = torch.linspace(0.0, 193.0 / GRID_ROWS, GRID_COLS)
        up = torch.nextafter(torch.tensor(20.0), torch.tensor(30.0))
        special = [0.0, 20.0, float(up), float(torch.tensor(1e-4)), -float(torch.tensor(1e-4)), 18.0]
        for i, v in enumerate(special):           # (the extra rows: x = (v, 0, ...), so z = v in every column; the rest of them z = 0)
            x[GRID_ROWS + i, 0] = v
        x, w = x.to(ops.device), w.to(ops.device)
        z = torch.empty(GRID_ROWS + EXTRA_ROWS, GRID_COLS, device=ops.device)
        y = ops.linear_act_fwd(x, w, None, act, z=z)
        y_alone = ops.linear_fwd(x, w, None, False, act=act)
        ident = ops.linear_fwd(x, w, None, False)
        _GRID[act] = (ops, x, w, y, z, y_alone, ident, special)
    return _GRID[act]


@pytest.mark.parametrize("act", ACTS)
def test_the_forward_on_the_grid_is_within_the_librarys_own_error_plus_one_ulp(act):
    ops, x, w, y, z, y_alone, ident, special = _grid(act)
    assert torch.equal(_bits(z), _bits(ident)) and torch.equal(_bits(y), _bits(y_alone))      # z the identity's bits, y the bits without z
    assert float(z.min()) <= -103.9 and float(z.max()) >= 89.0 and bool(torch.isfinite(z).all())
    for i, v in enumerate(special):
        assert float(z[GRID_ROWS + i, 0]) == v and float(z[GRID_ROWS + i, GRID_COLS - 1]) == v
    z64 = z.double()
    ref = _y64(act, z64)
    scale = torch.clamp(ref.abs(), min=TINY)
    own = ((y.double() - ref).abs() / scale).max() / ULP
    lib = ((_stock(act, z).double() - ref).abs() / scale).max() / ULP
    print("%s forward on the grid: max |y - y64(z)| / max(|y|, 2^-126): kernel %.3f ULP, library %.3f ULP (bar %.3f)"
          % (act, float(own), float(lib), BAR_Y[act]))
    assert float(own) <= BAR_Y[act] <= CAP


def test_softplus_gz_on_the_grid_is_within_the_librarys_own_error_plus_one_ulp():
    ops, _, _, y, _, _, _, _ = _grid("softplus")
    a = y.contiguous()                            # the outputs the forward gives over [-104, 89]: +0 up to 89
    assert float(a.min()) == 0.0 and float(a.max()) > 89.0
    g = _randn(GRID_ROWS + EXTRA_ROWS, GRID_COLS, 11)
    g[g.abs() < 1e-3] = 1e-3
    g = g.to(ops.device)
    w = (_randn(GRID_COLS, 64, 12) / 8).to(ops.device)
    gz, _ = ops.linear_bwd(g, a, w, act="softplus")
    ref = _gz64("softplus", g, a)
    own = ((gz.double() - ref).abs() / g.double().abs()).max() / ULP
    lib = (((g * (-torch.expm1(-a))).double() - ref).abs() / g.double().abs()).max() / ULP
    print("softplus g_z on the grid: max |gz - g (1 - e^-a)| / |g|: kernel %.3f ULP, library %.3f ULP (bar %.3f)"
          % (float(own), float(lib), BAR_SOFTPLUS_GZ))
    assert float(own) <= BAR_SOFTPLUS_GZ <= CAP
    assert torch.equal(_bits(gz[a >= 18.0]), _bits(g[a >= 18.0])) and int((a >= 18.0).sum()) > 1000
    assert bool((gz[a == 0] == 0).all()) and int((a == 0).sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------- forward
_FWD = {}


def _forward(act, rows, out_f, in_f, flags, bias):
    """Operands N(0, 1), w scaled by 3 in_f^-1/2 (z of a few units on either side of 0), and the act's, the identity's and the (y, z) results."""
    key = (act, rows, out_f, in_f, flags, bias)
    if key not in _FWD:
        ops = _ops()
        seed = tc.case_seed(rows, out_f, in_f)
        x = _randn(rows, in_f, seed).to(ops.device)
        w = (_randn(out_f, in_f, seed + 17) * 3.0 * in_f ** -0.5).to(ops.device)
        b = _randn(1, out_f, seed + 5).view(-1).to(ops.device) if bias else None
        ybuf, view = tc.guarded(rows, out_f, ops.device)
        y = ops.linear_fwd(x, w, b, False, view, flags=flags, act=act)
        ident = ops.linear_fwd(x, w, b, False, flags=flags)
        torch.cuda.synchronize()
        assert y is view and tc.guards_untouched(ybuf, rows) and ops.linear_fwd_supported(rows, out_f, in_f)
        _FWD[key] = (ops, x, w, b, y, ident)
    return _FWD[key]


def _exact(act, rows, out_f, in_f, flags, bias):
    """The exact small-integer operands of tests/test_gpu_linear_sigmoid.py: row HIGH_ROW has z = in_f + b >= 62 in columns 0 and 1, row
    LOW_ROW z = -2 in_f + b <= -126."""
    key = ("exact", act, rows, out_f, in_f, flags, bias)
    if key not in _FWD:
        ops = _ops()
        seed = tc.case_seed(rows, out_f, in_f)
        x, w = _randint(-4, 4, rows, in_f, seed) / 4, _randint(-2, 2, out_f, in_f, seed + 17) / 4
        x[HIGH_ROW], x[LOW_ROW] = 4.0, -8.0
        w[0], w[1] = 0.25, 0.25
        b = _randint(-8, 8, 1, out_f, seed + 5).view(-1) / 4 if bias else None
        x, w, b = x.to(ops.device), w.to(ops.device), None if b is None else b.to(ops.device)
        y = ops.linear_fwd(x, w, b, False, flags=flags, act=act)
        ident = ops.linear_fwd(x, w, b, False, flags=flags)
        _FWD[key] = (ops, x, w, b, y, ident)
    return _FWD[key]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_forward_is_the_activation_of_the_identity_forward_with_and_without_z(act, rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, ident = _forward(act, rows, out_f, in_f, flags, bias)
    assert bool(torch.isfinite(ident).all()) and bool((ident < -1).any()) and bool((ident > 1).any()) and float(ident.abs().max()) < 20.0
    ref = _y64(act, ident.double())
    err = ((y.double() - ref).abs() / torch.clamp(ref.abs(), min=TINY)).max() / ULP
    print("%s rows %d out %d in %d flags %d bias %s: max |y - y64(y_id)| / |y| = %.2f ULP" % (act, rows, out_f, in_f, flags, bias, float(err)))
    assert float(err) <= BAR_Y[act]
    if act == "elu":
        assert torch.equal(_bits(y[ident > 0]), _bits(ident[ident > 0])) and bool((y[ident <= 0] >= -1).all()) and bool((y[ident < 0] < 0).all())
    else:
        assert bool((y > 0).all()) and bool((y >= ident).all()) and bool((y[ident < 8] > ident[ident < 8]).all())
    # with z: the identity's bits beside the same y, inside their guards; a second launch gives the same bits
    zbuf, z = tc.guarded(rows, out_f, ops.device)
    ybuf, y2 = tc.guarded(rows, out_f, ops.device)
    out = ops.linear_act_fwd(x, w, b, act, y2, z, flags=flags)
    torch.cuda.synchronize()
    assert out is y2 and tc.guards_untouched(zbuf, rows) and tc.guards_untouched(ybuf, rows)
    assert torch.equal(_bits(z), _bits(ident)) and torch.equal(_bits(y2), _bits(y))
    assert torch.equal(_bits(ops.linear_act_fwd(x, w, b, act, flags=flags)), _bits(y))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_exact_operands_against_float64_and_the_two_saturated_rows(act, rows, out_f, in_f, flags, bias):
    ops, x, w, b, y, ident = _exact(act, rows, out_f, in_f, flags, bias)
    z64 = tc.forward64(x, w, b)
    z = z64.float()
    assert torch.equal(z.double(), z64) and torch.equal(ident, z)          # the premise: z is exact, and the identity kernel gives it
    ref = _y64(act, z64)
    err = ((y.double() - ref).abs() / torch.clamp(ref.abs(), min=TINY)).max() / ULP
    print("%s exact rows %d out %d in %d flags %d bias %s: %.2f ULP" % (act, rows, out_f, in_f, flags, bias, float(err)))
    assert float(err) <= BAR_Y[act]
    assert float(ident[HIGH_ROW, :2].min()) >= 62.0 and float(ident[LOW_ROW, :2].max()) <= -126.0
    high, low = ident >= 62.0, ident <= -126.0
    assert torch.equal(_bits(y[high]), _bits(ident[high]))
    if act == "softplus":
        assert bool((_bits(y[low]) == 0).all())                            # +0
    else:
        assert bool((y[low] == -1.0).all()) and torch.equal(_bits(y[ident > 0]), _bits(ident[ident > 0]))


@pytest.mark.parametrize("act", ACTS)
def test_random_operands_against_float64_within_twice_the_stock_pairs_own_error(act):
    worst = 0.0
    for rows, out_f, in_f, flags in FWD_CASES:
        for bias in (True, False):
            ops, x, w, b, y, _ = _forward(act, rows, out_f, in_f, flags, bias)
            ref = _y64(act, tc.forward64(x, w, b))
            scale = x.double().abs() @ w.double().abs().t()
            if b is not None:
                scale = scale + b.double().abs()
            lib = _stock(act, F.linear(x, w, b))
            e_own = float(((y.double() - ref).abs() / scale).max())
            e_lib = float(((lib.double() - ref).abs() / scale).max())
            worst = max(worst, e_own / e_lib)
            print("%s rows %d out %d in %d flags %d bias %d: pn_linear_fwd %.3e  stock %.3e  ratio %.2f"
                  % (act, rows, out_f, in_f, flags, bias, e_own, e_lib, e_own / e_lib))
            assert e_own <= MARGIN * e_lib, (act, rows, out_f, in_f, flags, bias, e_own, e_lib)
    print("%s worst ratio %.2f" % (act, worst))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rows,out_f,in_f,flags", FWD_CASES)
def test_a_nan_row_of_x_gives_a_nan_row_and_leaves_every_other_rows_bits(act, rows, out_f, in_f, flags):
    ops, x, w, b, y, _ = _forward(act, rows, out_f, in_f, flags, True)
    x2 = x.clone()
    x2[rows - 2] = float("nan")
    y2 = ops.linear_fwd(x2, w, b, False, flags=flags, act=act)
    others = torch.ones(rows, dtype=torch.bool, device=ops.device)
    others[rows - 2] = False
    assert bool(torch.isnan(y2[rows - 2]).all()) and torch.equal(_bits(y2[others]), _bits(y[others]))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("bias", [True, False])
def test_the_forward_has_the_same_bits_in_every_form(act, bias):
    ops, x, w, b, y, _ = _forward(act, 256, 128, 64, 0, bias)
    _, x1, w1, b1, y_plain, _ = _forward(act, 256, 128, 64, PLAIN, bias)
    assert torch.equal(x, x1) and torch.equal(w, w1) and torch.equal(_bits(y), _bits(y_plain))
    x300 = torch.cat([x, _randn(44, 64, 99).to(ops.device)])               # the ragged body: 300 rows whose first 256 are these
    z300 = torch.empty(300, 128, device=ops.device)
    y300 = ops.linear_fwd(x300, w, b, False, act=act)
    assert not tc.is_aligned(300, 128) and torch.equal(_bits(y300[:256]), _bits(y))
    assert torch.equal(_bits(ops.linear_act_fwd(x300, w, b, act, z=z300)[:256]), _bits(y))


# ------------------------------------------------------------------------------------------------------------------------ backward
_BWD = {}


def _outputs(act, rows, k, seed, nans):
    """The pair's output as the kernel may meet it.  Softplus: values above 0, exact zeros, values of 18 and more.  ELU: values of (-1, 0]
    and above 0, exact -1 and +-0.  With `nans`, a few NaNs."""
    pick = torch.randint(0, 8, (rows, k), generator=torch.Generator().manual_seed(seed + 1))
    if act == "softplus":
        a = F.softplus(4.0 * _randn(rows, k, seed))
        a[pick == 0] = 0.0
        a[pick == 1] = 18.0
        a[pick == 2] = 40.0
    else:
        a = F.elu(2.0 * _randn(rows, k, seed))
        a[pick == 0] = 0.0
        a[pick == 1] = -1.0
        a[pick == 2] = -0.0
    if nans:
        a[16:24][pick[16:24] == 3] = float("nan")                 # (eight rows of them; the other rows stay clean)
        a[0, 0], a[rows - 1, k - 1] = float("nan"), float("nan")
    return a


def _backward(act, rows, out_f, in_f, flags):
    key = (act, rows, out_f, in_f, flags)
    if key not in _BWD:
        ops = _ops()
        seed = tc.case_seed(rows, in_f, out_f)
        g = _randn(rows, out_f, seed)
        g[g.abs() < 1e-3] = 1e-3                   # (the normal range, well away from a product that underflows)
        g = g.to(ops.device)
        w = (_randn(out_f, in_f, seed + 17) * out_f ** -0.5).to(ops.device)
        a = _outputs(act, rows, out_f, seed + 3, False).to(ops.device)
        gbuf, gz = tc.guarded(rows, out_f, ops.device)
        dbuf, dx = tc.guarded(rows, in_f, ops.device)
        out = ops.linear_bwd(g, a, w, gz, dx, flags=flags, act=act)
        torch.cuda.synchronize()
        assert out[0] is gz and out[1] is dx and ops.linear_bwd_supported(rows, out_f, in_f)
        _BWD[key] = (ops, g, a, w, gbuf, gz, dbuf, dx)
    return _BWD[key]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_gz_meets_its_bars_and_dx_has_the_bits_of_pn_linear_dx_fed_gz(act, rows, out_f, in_f, flags):
    ops, g, a, w, gbuf, gz, dbuf, dx = _backward(act, rows, out_f, in_f, flags)
    err = (gz.double() - _gz64(act, g, a)).abs() / g.double().abs() / ULP
    print("%s rows %d out %d in %d flags %d: max |gz - gz64| / |g| = %.2f ULP" % (act, rows, out_f, in_f, flags, float(err.max())))
    if act == "softplus":
        assert float(err.max()) <= BAR_SOFTPLUS_GZ
        big = a >= 18.0
        assert int(big.sum()) > 100 and torch.equal(_bits(gz[big]), _bits(g[big])) and bool((gz[a == 0] == 0).all()) and bool((a == 0).any())
        assert bool(((gz - g * (-torch.expm1(-a))).abs() <= 4.0 * ULP * g.abs()).all())       # the engine's self-check bar
    else:
        pos = a > 0
        assert int(pos.sum()) > 100 and torch.equal(_bits(gz[pos]), _bits(g[pos]))
        assert float(err[~pos].max()) <= 1.5 and bool((gz[a == -1.0] == 0).all()) and bool((a == -1.0).any())
        assert torch.equal(_bits(gz[a == 0]), _bits(g[a == 0])) and bool((_bits(a) == -2 ** 31).any())       # a == +-0: a + 1 is 1
        assert bool(((gz - torch.ops.aten.elu_backward(g, 1, 1, 1, True, a)).abs() <= 1.5 * ULP * g.abs()).all())
    # dx: the bits of pn_linear_dx fed that gz, within the engine's bar of float64
    want = ops.linear_dx(gz.contiguous(), w, flags=flags)
    assert dx.shape == (rows, in_f) and torch.equal(_bits(dx), _bits(want)), int((dx != want).sum())
    ref = gz.double() @ w.double()
    assert bool(((dx.double() - ref).abs() <= CHECK_TOL * (gz.double().abs() @ w.double().abs())).all())
    # sentinels, and a second launch gives the same bits
    assert tc.guards_untouched(gbuf, rows) and tc.guards_untouched(dbuf, rows)
    gbuf2, gz2 = tc.guarded(rows, out_f, ops.device)
    dbuf2, dx2 = tc.guarded(rows, in_f, ops.device)
    ops.linear_bwd(g, a, w, gz2, dx2, flags=flags, act=act)
    torch.cuda.synchronize()
    assert tc.guards_untouched(gbuf2, rows) and tc.guards_untouched(dbuf2, rows)
    assert torch.equal(_bits(gz2), _bits(gz)) and torch.equal(_bits(dx2), _bits(dx))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("rows,out_f,in_f,flags", BWD_CASES)
def test_a_nan_or_an_infinite_g_stays_in_its_element_of_gz_and_its_row_of_dx(act, rows, out_f, in_f, flags):
    ops, g, a, w, _, gz, _, dx = _backward(act, rows, out_f, in_f, flags)
    a2 = _outputs(act, rows, out_f, tc.case_seed(rows, in_f, out_f) + 3, True).to(ops.device)
    g2 = g.clone()
    g2[7, 3], g2[9, 1], g2[11, 2], a2[9, 1], a2[11, 2] = float("nan"), float("inf"), -float("inf"), 1.0, 0.5
    odd = torch.isnan(a2) | ~torch.isfinite(g2)
    assert int(odd.sum()) > 4
    gz2, dx2 = ops.linear_bwd(g2, a2, w, flags=flags, act=act)
    assert not bool(torch.isfinite(gz2[odd]).any()) and bool(torch.isfinite(gz2[~odd]).all())
    assert bool(torch.isnan(gz2[torch.isnan(a2) | torch.isnan(g2)]).all())            # a NaN in a gives a NaN in gz: ELU's comparison is a > 0
    assert float(gz2[9, 1]) == float("inf") and float(gz2[11, 2]) == -float("inf")
    rows_odd = odd.any(1)
    assert not bool(torch.isfinite(dx2[rows_odd]).any()) and not bool(rows_odd.all())
    # a clean row's gz and dx depend on that row alone
    clean = ~rows_odd
    a3, g3 = a2.clone(), g2.clone()
    a3[rows_odd], g3[rows_odd] = 0.5, 1.0
    gz3, dx3 = ops.linear_bwd(g3, a3, w, flags=flags, act=act)
    assert torch.equal(_bits(dx2[clean]), _bits(dx3[clean])) and torch.equal(_bits(gz2[clean]), _bits(gz3[clean]))
    assert bool(torch.isfinite(dx2[clean]).all())


@pytest.mark.parametrize("act", ACTS)
def test_gz_and_dx_have_the_same_bits_in_every_form(act):
    ops, g, a, w, _, gz, _, dx = _backward(act, 256, 64, 128, 0)
    _, g1, a1, w1, _, gz_plain, _, dx_plain = _backward(act, 256, 64, 128, PLAIN)
    assert torch.equal(g, g1) and torch.equal(a, a1) and torch.equal(w, w1)
    assert torch.equal(_bits(gz), _bits(gz_plain)) and torch.equal(_bits(dx), _bits(dx_plain))
    g300 = torch.cat([g, _randn(44, 64, 98).to(ops.device)])               # the ragged body: 300 rows whose first 256 are these
    a300 = torch.cat([a, _outputs(act, 44, 64, 97, False).to(ops.device)])
    gz300, dx300 = ops.linear_bwd(g300, a300, w, act=act)
    assert torch.equal(_bits(gz300[:256]), _bits(gz)) and torch.equal(_bits(dx300[:256]), _bits(dx))


def _act(ops, g, a, w, act, gz, dx, flags, rows=None, out_f=None, in_f=None):
    """pn_linear_bwd_act as it is exported; tensors or raw addresses."""
    def ptr(v):
        return v.data_ptr() if isinstance(v, torch.Tensor) else v
    rows = g.shape[0] if rows is None else rows
    out_f = w.shape[0] if out_f is None else out_f
    in_f = w.shape[1] if in_f is None else in_f
    return ops.lib.pn_linear_bwd_act(ops.stream(), ops.code, rows, out_f, in_f, ptr(g), ptr(a), ptr(w), act, ptr(gz), ptr(dx), flags)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("flags", [0, PLAIN])
def test_refused_calls_return_nonzero_and_leave_the_outputs_untouched(act, flags):
    from pnode_amd import _lib
    from pnode_amd._lib import PnError
    ops = _ops()
    CODE = {"softplus": _lib.PN_ACT_SOFTPLUS, "elu": _lib.PN_ACT_ELU}[act]
    rows, out_f, in_f = 256, 64, 128
    g = torch.full((rows, out_f), 8.0, device=ops.device)
    a = torch.full((rows, out_f), 25.0 if act == "softplus" else -0.5, device=ops.device)
    w = torch.full((out_f, in_f), 5.0, device=ops.device)
    gbuf, gz = tc.guarded(rows, out_f, ops.device)
    dbuf, dx = tc.guarded(rows, in_f, ops.device)
    xbuf, xy = tc.guarded(rows, in_f, ops.device)             # a forward output: y of x = g (256 x 64) and w^T (128 x 64)
    zbuf, xz = tc.guarded(rows, in_f, ops.device)
    wt = w.t().contiguous()

    def untouched():
        torch.cuda.synchronize()
        words = (gbuf.view(torch.int32), dbuf.view(torch.int32), xbuf.view(torch.int32), zbuf.view(torch.int32))
        return all(bool((v == tc.SENTINEL).all()) for v in words) and bool((g == 8.0).all()) and bool((a == a[0, 0]).all()) and bool((w == 5.0).all())

    def last():
        return ops.lib.pn_last_error().decode()

    def ptr(v):
        return v.data_ptr() if isinstance(v, torch.Tensor) else v

    def fwd(code, y, x=g, rows_=rows, in_=out_f, z=None):
        if z is not None:
            return ops.lib.pn_linear_fwd_pre(ops.stream(), ops.code, rows_, in_f, in_, ptr(x), wt.data_ptr(), None, code, ptr(y), ptr(z), flags)
        return ops.lib.pn_linear_fwd_form(ops.stream(), ops.code, rows_, in_f, in_, ptr(x), wt.data_ptr(), None, code, ptr(y), flags)

    for bad in (6, 9, 17, 33, 48, 3, -1):
        assert _act(ops, g, a, w, bad, gz, dx, flags) != 0 and "or PN_ACT_SOFTPLUS or PN_ACT_ELU (PN_ACT_IDENTITY: use pn_linear_dx)" in last()
        assert fwd(bad, xy) != 0 and "or PN_ACT_GELU or PN_ACT_SOFTPLUS or PN_ACT_ELU" in last()
        assert fwd(bad, xy, z=xz) != 0 and "or PN_ACT_GELU or PN_ACT_SOFTPLUS or PN_ACT_ELU" in last()
    assert untouched()
    assert _act(ops, g, a, w, CODE, gz, dx, flags | 2) != 0 and "pn_linear_bwd_act: unknown flag" in last() and untouched()
    assert _act(ops, g, a, w, CODE, g, dx, flags) != 0 and "gz must not alias" in last() and untouched()
    w64 = torch.full((64, 64), 5.0, device=ops.device)
    assert _act(ops, g, a, w64, CODE, gz, gz, flags) != 0 and "dx must not alias" in last() and untouched()
    assert fwd(CODE, g) != 0 and "y must not alias" in last() and untouched()
    assert fwd(CODE, xy, z=xy) != 0 and "z must not alias" in last() and fwd(CODE, xy, z=0) != 0 and untouched()
    for k in range(5):
        for bad in (lambda v: v.data_ptr() + 4, lambda v: None):
            args = [g, a, w, gz, dx]
            args[k] = bad(args[k])
            assert _act(ops, args[0], args[1], args[2], CODE, args[3], args[4], flags, rows, out_f, in_f) != 0
            assert "16-byte aligned" in last() or "null operand" in last()
    assert fwd(CODE, xy.data_ptr() + 4) != 0 and "16-byte aligned" in last() and fwd(CODE, xy, x=None) != 0 and "null operand" in last()
    assert untouched()
    for r, o, i in ((255, out_f, in_f), (128, out_f, in_f), (rows, 80, in_f), (rows, 48, in_f), (rows, out_f, 100)):
        assert not ops.linear_bwd_supported(r, o, i)
        assert _act(ops, g, a, w, CODE, gz, dx, flags, r, o, i) != 0 and "unsupported dtype or shape" in last()
    for r, k in ((255, out_f), (rows, 80)):
        assert not ops.linear_fwd_supported(r, in_f, k)
        assert fwd(CODE, xy, rows_=r, in_=k) != 0 and "unsupported dtype or shape" in last()
    assert ops.lib.pn_linear_bwd_act(ops.stream(), 1, rows, out_f, in_f, g.data_ptr(), a.data_ptr(), w.data_ptr(), CODE, gz.data_ptr(),
                                     dx.data_ptr(), flags) != 0 and "unsupported dtype or shape" in last()
    assert untouched()
    # the backend refuses an activation it does not know, by name, before any launch
    with pytest.raises(PnError, match="tanh or relu or sigmoid or gelu or softplus or elu"):
        ops.linear_bwd(g, a, w, gz, dx, flags=flags, act="identity")
    with pytest.raises(PnError, match="identity, tanh or relu or sigmoid or softplus or elu"):
        ops.linear_fwd(g, wt, None, False, flags=flags, act="silu")
    with pytest.raises(PnError, match="identity, tanh or relu or sigmoid or gelu or softplus or elu"):
        ops.linear_act_fwd(g, wt, None, "silu", flags=flags)
    assert untouched()
    # and the same operands, not aliased, go through, all exact: Softplus a = 25: gz = g = 8, dx = 64 * 8 * 5; ELU a = -1/2: gz = 4,
    # dx = 64 * 4 * 5; the forward of x = 8, w = 5 over K = 64 is z = 2560 = y in both
    assert _act(ops, g, a, w, CODE, gz, dx, flags) == 0 and fwd(CODE, xy, z=xz) == 0
    torch.cuda.synchronize()
    want = 8.0 if act == "softplus" else 4.0
    assert bool((gz == want).all()) and bool((dx == out_f * want * 5.0).all()) and bool((xy == 2560.0).all()) and bool((xz == 2560.0).all())
    assert tc.guards_untouched(gbuf, rows) and tc.guards_untouched(dbuf, rows) and tc.guards_untouched(xbuf, rows) and tc.guards_untouched(zbuf, rows)
