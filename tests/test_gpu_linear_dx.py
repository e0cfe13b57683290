"""-m gpu: pn_linear_dx (csrc/pn_linear.hip), dx = g w for a bare Linear layer, through HipVecOps.

Shapes (rows, out_f, in_f), the smallest that reach every instantiation: 256 x 64 x 128 aligned, two K slabs: pipelined (and, asked for, plain);
256 x 128 x 128 four slabs; 256 x 96 x 128 three slabs -- an odd number: the plain loop; 320 x 64 x 64 ragged in rows and columns;
256 x 64 x 192 ragged in columns only.  Each with flags 0 and PN_LINEAR_FORM_PLAIN.

The contract is bits: dx equals the dx of pn_linear_bwd(g, a = 0, w) -- the tanh body fed zeros, g (1 - 0 0) == g -- in every shape and
form.  On operands whose every partial sum is exact in fp32 (tests/_linear_tile_cases.py: `distinct`) dx is the float64 product bit for
bit, and powers of two scale it bit for bit.  On random operands the error against float64 in units of |g| |w| is at most MARGIN = 2 times
the library matmul's own on the same operands (the bar of tests/test_gpu_linear_fwd.py and test_gpu_linear_forms.py: the split product
rounds less than an fp32 chain; the margin covers the library summing more favourably at some shape).
Measured on MI355X, worst over the ten cases: pn_linear_dx 1.35e-7 against the library's 2.73e-7, ratios within a case 0.45 to 0.58."""
import pytest
import torch

import _linear_tile_cases as tc
from conftest import require_gpu

pytestmark = pytest.mark.gpu

PLAIN = 1                             # PN_LINEAR_FORM_PLAIN
SHAPES = [(256, 64, 128), (256, 128, 128), (256, 96, 128), (320, 64, 64), (256, 64, 192)]
RAGGED = [(320, 64, 64), (256, 64, 192)]
FLAGS = [0, PLAIN]
MARGIN = 2.0


def _ops():
    from pnode_amd import _lib
    from pnode_amd._vecops import HipVecOps
    assert _lib.PN_LINEAR_FORM_PLAIN == PLAIN
    return HipVecOps(require_gpu(), torch.float32, 320 * 192)


def _seed(rows, out_f, in_f):
    return tc.case_seed(rows, in_f, out_f)


def _operands(kind, rows, out_f, in_f, dev):
    """g (rows, out_f), w (out_f, in_f) as tests/_linear_tile_cases.py builds the backward's (width = in_f, K = out_f)."""
    g, _, w = tc.backward_operands(kind, rows, in_f, out_f, _seed(rows, out_f, in_f))
    return g.to(dev), w.to(dev)


def test_the_shapes_reach_every_instantiation():
    kinds = set()
    for rows, out_f, in_f in SHAPES:
        if not tc.is_aligned(rows, in_f):
            kinds.add("ragged")
        else:
            kinds.add("pipelined" if tc.pipelines(out_f) else "plain")
    assert kinds == {"ragged", "pipelined", "plain"}
    assert all(not tc.is_aligned(r, i) for r, _, i in RAGGED)


@pytest.mark.parametrize("kind", ["distinct", "normal"])
@pytest.mark.parametrize("rows,out_f,in_f", SHAPES)
def test_dx_has_the_bits_of_the_tanh_kernel_fed_zeros_in_every_form(rows, out_f, in_f, kind):
    ops = _ops()
    g, w = _operands(kind, rows, out_f, in_f, ops.device)
    zeros = torch.zeros_like(g)
    got = {}
    for flags in FLAGS:
        dx = ops.linear_dx(g, w, flags=flags)
        assert dx.shape == (rows, in_f) and dx.dtype == torch.float32
        gz, want = ops.linear_bwd(g, zeros, w, flags=flags)
        assert torch.equal(gz, g)
        assert torch.equal(dx.view(torch.int32), want.view(torch.int32)), (flags, int((dx != want).sum()))
        got[flags] = dx
    assert torch.equal(got[0].view(torch.int32), got[PLAIN].view(torch.int32))
    assert ops.linear_dx_supported(rows, out_f, in_f) and ops.linear_bwd_supported(rows, out_f, in_f)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("rows,out_f,in_f", SHAPES)
def test_exact_operands_give_the_float64_product_and_powers_of_two_scale_it_bit_for_bit(rows, out_f, in_f, flags):
    ops = _ops()
    g, w = _operands("distinct", rows, out_f, in_f, ops.device)
    want = (g.double() @ w.double())
    assert torch.equal(want.float().double(), want)                  # an fp32 number, whatever the order of the sum
    dx = ops.linear_dx(g, w, flags=flags)
    bad = tc.first_wrong_tile(dx.cpu(), want.float().cpu())
    assert bad is None, bad
    for p, q in tc.SCALINGS:
        dxs = ops.linear_dx(g * 2.0 ** p, w * 2.0 ** q, flags=flags)
        assert torch.equal(dxs.view(torch.int32), (dx * 2.0 ** (p + q)).view(torch.int32)), (p, q)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("rows,out_f,in_f", SHAPES)
def test_random_operands_are_as_close_to_float64_as_the_library_matmul(rows, out_f, in_f, flags):
    ops = _ops()
    g, w = _operands("normal", rows, out_f, in_f, ops.device)
    ref = g.double() @ w.double()
    scale = g.double().abs() @ w.double().abs()
    dx = ops.linear_dx(g, w, flags=flags)
    lib = torch.matmul(g, w)
    e_own = float(((dx.double() - ref).abs() / scale).max())
    e_lib = float(((lib.double() - ref).abs() / scale).max())
    print("rows %d out %d in %d flags %d: pn_linear_dx %.3e  library %.3e  ratio %.2f" % (rows, out_f, in_f, flags, e_own, e_lib, e_own / e_lib))
    assert e_own <= MARGIN * e_lib, (e_own, e_lib)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("rows,out_f,in_f", [(256, 64, 128), (320, 64, 64)])
def test_nan_and_inf_stay_in_their_row_and_an_inf_in_w_in_the_columns_it_feeds(rows, out_f, in_f, flags):
    ops = _ops()
    g, w = _operands("normal", rows, out_f, in_f, ops.device)
    dx0 = ops.linear_dx(g, w, flags=flags)
    assert bool(torch.isfinite(dx0).all())
    g2 = g.clone()
    g2[17, 5] = float("nan")
    g2[rows - 1, out_f - 1] = float("inf")
    dx = ops.linear_dx(g2, w, flags=flags)
    others = torch.ones(rows, dtype=torch.bool, device=ops.device)
    others[17] = others[rows - 1] = False
    assert torch.equal(dx[others].view(torch.int32), dx0[others].view(torch.int32))
    assert bool(torch.isnan(dx[17]).all()) and not bool(torch.isfinite(dx[rows - 1]).any())
    w2 = w.clone()
    w2[3, 9] = float("inf")
    w2[out_f - 1, in_f - 1] = float("-inf")
    dx = ops.linear_dx(g, w2, flags=flags)
    cols = torch.ones(in_f, dtype=torch.bool, device=ops.device)
    cols[9] = cols[in_f - 1] = False
    assert torch.equal(dx[:, cols].view(torch.int32), dx0[:, cols].view(torch.int32))
    assert not bool(torch.isfinite(dx[:, ~cols]).any())


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("rows,out_f,in_f", SHAPES)
def test_repeated_launches_into_rotating_buffers_give_the_same_bits(rows, out_f, in_f, flags):
    ops = _ops()
    g, w = _operands("normal", rows, out_f, in_f, ops.device)
    first = ops.linear_dx(g, w, flags=flags).clone()
    bufs = [torch.full((rows, in_f), float("nan"), device=ops.device) for _ in range(3)]
    for k in range(9):
        out = ops.linear_dx(g, w, bufs[k % 3], flags=flags)
        assert out is bufs[k % 3]
    for b in bufs:
        assert torch.equal(b.view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("rows,out_f,in_f", RAGGED)
def test_the_guard_bands_around_dx_are_unchanged_in_the_ragged_shapes(rows, out_f, in_f, flags):
    ops = _ops()
    g, w = _operands("distinct", rows, out_f, in_f, ops.device)
    buf, view = tc.guarded(rows, in_f, ops.device)
    ops.linear_dx(g, w, view, flags=flags)
    torch.cuda.synchronize()
    assert tc.guards_untouched(buf, rows)
    assert torch.equal(view.cpu(), (g.double() @ w.double()).float().cpu())


def _off16(t):
    """A contiguous copy of t that starts at element 1 of a larger buffer: 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 4, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _is(t, value):
    torch.cuda.synchronize()
    return bool((t == value).all())


@pytest.mark.parametrize("flags", FLAGS)
def test_aliased_misaligned_fp64_and_small_calls_are_refused_with_dx_unchanged(flags):
    """Every refused call launches nothing."""
    from pnode_amd._lib import PnError
    ops = _ops()
    # dx is g (256 x 64 x 64: the two have one shape)
    g = torch.full((256, 64), 7.0, device=ops.device)
    w = torch.full((64, 64), 5.0, device=ops.device)
    dx = torch.full((256, 64), 9.0, device=ops.device)
    with pytest.raises(PnError, match="alias"):
        ops.linear_dx(g, w, g, flags=flags)
    assert _is(g, 7.0)
    # dx is w (256 x 256 x 64: the two have one shape)
    g2 = torch.full((256, 256), 7.0, device=ops.device)
    w2 = torch.full((256, 64), 5.0, device=ops.device)
    with pytest.raises(PnError, match="alias"):
        ops.linear_dx(g2, w2, w2, flags=flags)
    assert _is(w2, 5.0)
    # a pointer off 16 bytes: each operand in turn
    for args in ((_off16(g), w, dx), (g, _off16(w), dx)):
        with pytest.raises(PnError, match="aligned"):
            ops.linear_dx(*args, flags=flags)
        assert _is(dx, 9.0)
    dx1 = _off16(dx)
    with pytest.raises(PnError, match="aligned"):
        ops.linear_dx(g, w, dx1, flags=flags)
    assert _is(dx1, 9.0)
    # an fp64 state: its code, and its tensors
    ops64 = _ops()
    ops64.code = 1
    assert not ops64.linear_dx_supported(256, 64, 64)
    with pytest.raises(PnError):
        ops64.linear_dx(g, w, dx, flags=flags)
    dx64 = dx.double()
    with pytest.raises(PnError):
        ops.linear_dx(g.double(), w.double(), dx64, flags=flags)
    assert _is(dx, 9.0) and _is(dx64, 9.0)
    # rows of 128
    assert not ops.linear_dx_supported(128, 64, 64)
    small = torch.full((128, 64), 9.0, device=ops.device)
    with pytest.raises(PnError, match="unsupported"):
        ops.linear_dx(g[:128], w, small, flags=flags)
    assert _is(small, 9.0)
    # an unknown flag, whatever else holds
    with pytest.raises(PnError, match="unknown flag"):
        ops.linear_dx(g, w, dx, flags=2 | flags)
    assert _is(dx, 9.0)
    # and the same operands, not aliased, go through
    out = ops.linear_dx(g, w, dx, flags=flags)
    assert out is dx and _is(dx, 64 * 7.0 * 5.0)
