"""-m gpu: pn_linear_bwd (csrc/pn_linear.hip), gz = g (1 - a^2) and dx = gz w in one launch, through HipVecOps against float64.

Shapes: rows 256 / 320 (ragged: no multiple of the 64-row tile) / 384; (out_f, in_f) = (64, 64) two K slabs, the 128-wide tile half empty;
(64, 192) two column tiles -- only the first writes gz; (192, 64) six slabs; (256, 128) one full tile, eight slabs.

gz: within 3 * 2^-24 |g| of the float64 value, elementwise (two roundings in 1 - a^2, one in the product, with or without an fma).
dx: judged against the float64 product of the kernel's OWN gz, so that only the product is judged; measure max |err| / (|gz| @ |w|); the bar
is the library's error, torch.matmul(gz_own, w) in fp32 on the same operands in the same measure, times MARGIN = 1.5: the split product rounds
less than an fp32 chain (5.7e-8 against 1.0e-7) and the forward's identity cases measured a worst ratio of 0.66; the
margin only covers the library choosing a more favourable summation at some shape.
Measured on MI355X, worst over the 12 cases: gz 8.9e-8 |g| (half the bar); dx pn_linear_bwd 1.89e-7 against the library's 3.07e-7, worst
ratio within a case 0.73 (rows 320, 64 x 64)."""
import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu

ROWS = [256, 320, 384]
SHAPES = [(64, 64), (64, 192), (192, 64), (256, 128)]
MARGIN = 1.5
GZ_TOL = 3.0 * 2.0 ** -24


def _ops(rows, out_f):
    from pnode_amd._vecops import HipVecOps
    return HipVecOps(require_gpu(), torch.float32, rows * out_f)


def _gz64(g, a):
    return g.double() * (1.0 - a.double() * a.double())


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("out_f,in_f", SHAPES)
def test_exact_operands_give_the_float64_results(rows, out_f, in_f):
    """g multiples of 4 in [-16, 16], a in {0, +-0.5, +-1}: 1 - a^2 in {1, 0.75, 0}, gz an integer of at most 5 bits; w integers in
    [-4, 4]: every term and every partial sum is exact in any order."""
    ops = _ops(rows, out_f)
    gen = torch.Generator().manual_seed(rows + 7 * out_f + in_f)
    g = (4 * torch.randint(-4, 5, (rows, out_f), generator=gen)).float().to(ops.device)
    a = (torch.randint(-2, 3, (rows, out_f), generator=gen).float() / 2).to(ops.device)
    w = torch.randint(-4, 5, (out_f, in_f), generator=gen).float().to(ops.device)
    g[::5] = 0
    a[3::7] = 0
    gz64 = _gz64(g, a)
    dx64 = gz64 @ w.double()
    gz, dx = ops.linear_bwd(g, a, w)
    assert gz.shape == (rows, out_f) and dx.shape == (rows, in_f)
    assert torch.equal(gz, gz64.float()), float((gz.double() - gz64).abs().max())
    assert torch.equal(dx, dx64.float()), float((dx.double() - dx64).abs().max())
    assert not bool(dx[::5].any())


@pytest.fixture(scope="module")
def worst():
    seen = {"ratio": 0.0, "own": 0.0, "lib": 0.0}
    yield seen
    print("\npn_linear_bwd dx, worst over the cases run: own %.3e  library %.3e  worst ratio within a case %.2f" % (seen["own"], seen["lib"], seen["ratio"]))


def _random(rows, out_f, in_f, dev):
    gen = torch.Generator().manual_seed(3 * rows + out_f + 11 * in_f)
    a = torch.tanh(torch.randn(rows, out_f, generator=gen)).to(dev)
    g = torch.randn(rows, out_f, generator=gen).to(dev)
    w = (torch.randn(out_f, in_f, generator=gen) / out_f ** 0.5).to(dev)
    return g, a, w


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("out_f,in_f", SHAPES)
def test_random_operands_gz_is_within_three_roundings_of_float64(rows, out_f, in_f):
    ops = _ops(rows, out_f)
    g, a, w = _random(rows, out_f, in_f, ops.device)
    gz, _ = ops.linear_bwd(g, a, w)
    err = (gz.double() - _gz64(g, a)).abs()
    print("rows %d out %d in %d: max |gz - gz64| / |g| = %.3e (allowed %.3e)" % (rows, out_f, in_f, float((err / g.double().abs()).max()), GZ_TOL))
    assert bool((err <= GZ_TOL * g.double().abs()).all())


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("out_f,in_f", SHAPES)
def test_random_operands_dx_is_as_close_to_float64_as_the_library_product(rows, out_f, in_f, worst):
    ops = _ops(rows, out_f)
    g, a, w = _random(rows, out_f, in_f, ops.device)
    gz, dx = ops.linear_bwd(g, a, w)
    ref = gz.double() @ w.double()
    scale = gz.double().abs() @ w.double().abs()
    lib = torch.matmul(gz, w)
    e_own = float(((dx.double() - ref).abs() / scale).max())
    e_lib = float(((lib.double() - ref).abs() / scale).max())
    print("rows %d out %d in %d: pn_linear_bwd %.3e  library %.3e  ratio %.2f" % (rows, out_f, in_f, e_own, e_lib, e_own / e_lib))
    worst["ratio"], worst["own"], worst["lib"] = max(worst["ratio"], e_own / e_lib), max(worst["own"], e_own), max(worst["lib"], e_lib)
    assert e_own <= MARGIN * e_lib, (e_own, e_lib)


def test_nan_inf_and_saturated_rows_stay_in_their_rows_and_launches_repeat_bitwise():
    rows, out_f, in_f = 320, 64, 192
    ops = _ops(rows, out_f)
    g, a, w = _random(rows, out_f, in_f, ops.device)
    gz0, dx0 = ops.linear_bwd(g, a, w)
    gz1, dx1 = ops.linear_bwd(g, a, w)
    assert torch.equal(gz0, gz1) and torch.equal(dx0, dx1)
    assert bool(torch.isfinite(gz0).all()) and bool(torch.isfinite(dx0).all())
    # a NaN in g[17, 5]
    g2 = g.clone()
    g2[17, 5] = float("nan")
    gz, dx = ops.linear_bwd(g2, a, w)
    others = torch.ones(rows, dtype=torch.bool, device=ops.device)
    others[17] = False
    assert torch.equal(gz[others], gz0[others]) and torch.equal(dx[others], dx0[others])
    assert bool(torch.isnan(gz[17, 5])) and torch.equal(gz[17, :5], gz0[17, :5]) and torch.equal(gz[17, 6:], gz0[17, 6:])
    assert bool(torch.isnan(dx[17]).all())
    # rows with a = +-1 everywhere
    a2 = a.clone()
    a2[40] = 1.0
    a2[319] = -1.0
    a2[100, ::2] = 1.0
    a2[100, 1::2] = -1.0
    gz, dx = ops.linear_bwd(g, a2, w)
    sat = torch.zeros(rows, dtype=torch.bool, device=ops.device)
    sat[40] = sat[319] = sat[100] = True
    assert bool((gz[sat] == 0).all()) and bool((dx[sat] == 0).all())
    assert torch.equal(gz[~sat], gz0[~sat]) and torch.equal(dx[~sat], dx0[~sat])
    # an Inf in g[300, 63]
    g3 = g.clone()
    g3[300, 63] = float("inf")
    gz, dx = ops.linear_bwd(g3, a, w)
    others = torch.ones(rows, dtype=torch.bool, device=ops.device)
    others[300] = False
    assert bool(torch.isinf(gz[300, 63])) and not bool(torch.isfinite(dx[300]).any())
    assert torch.equal(gz[others], gz0[others]) and torch.equal(dx[others], dx0[others])


def _prefilled(rows, out_f, in_f, dev):
    return torch.full((rows, out_f), 7.0, device=dev), torch.full((rows, in_f), 9.0, device=dev)


def _untouched(gz, dx):
    torch.cuda.synchronize()
    return bool((gz == 7.0).all()) and bool((dx == 9.0).all())


@pytest.mark.parametrize("rows,out_f,in_f", [(255, 64, 64), (256, 80, 64), (256, 32, 64), (256, 64, 96)])
def test_unsupported_shapes_are_refused_and_nothing_is_launched(rows, out_f, in_f):
    from pnode_amd._lib import PnError
    ops = _ops(rows, out_f)
    assert not ops.linear_bwd_supported(rows, out_f, in_f)
    g = torch.ones(rows, out_f, device=ops.device)
    a = torch.zeros(rows, out_f, device=ops.device)
    w = torch.ones(out_f, in_f, device=ops.device)
    gz, dx = _prefilled(rows, out_f, in_f, ops.device)
    with pytest.raises(PnError):
        ops.linear_bwd(g, a, w, gz, dx)
    assert _untouched(gz, dx)


def test_an_fp64_state_and_aliased_outputs_are_refused_and_nothing_is_launched():
    from pnode_amd._lib import PnError
    rows, out_f, in_f = 256, 64, 64
    ops = _ops(rows, out_f)
    assert ops.linear_bwd_supported(rows, out_f, in_f)
    g = torch.full((rows, out_f), 7.0, device=ops.device)
    a = torch.full((rows, out_f), 9.0, device=ops.device)
    w = torch.ones(out_f, in_f, device=ops.device)
    gz, dx = _prefilled(rows, out_f, in_f, ops.device)
    # an fp64 state: its code, and its tensors
    ops64 = _ops(rows, out_f)
    ops64.code = 1
    assert not ops64.linear_bwd_supported(rows, out_f, in_f)
    with pytest.raises(PnError):
        ops64.linear_bwd(g, a, w, gz, dx)
    with pytest.raises(PnError):
        ops.linear_bwd(g.double(), a.double(), w.double(), gz.double(), dx.double())
    assert _untouched(gz, dx)
    # gz is g (g holds 7 as well: untouched reads the same); dx aliasing a (a holds 9)
    with pytest.raises(PnError):
        ops.linear_bwd(g, a, w, g, dx)
    assert _untouched(g, dx)
    with pytest.raises(PnError):
        ops.linear_bwd(g, a, w, gz, a)
    assert _untouched(gz, a)
    # and the same operands, not aliased, go through
    gz, dx = ops.linear_bwd(g, a, w, gz, dx)
    torch.cuda.synchronize()
    assert bool((gz == 7.0 * (1.0 - 81.0)).all()) and bool((dx == 64 * 7.0 * (1.0 - 81.0)).all())
