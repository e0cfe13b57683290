"""-m gpu: the index arithmetic of pn_linear_fwd / pn_linear_bwd (csrc/pn_linear.hip) at the edges, through HipVecOps.  Everything compares
bits or exact values; operands and shapes are tests/_linear_tile_cases.py (checked on the CPU by tests/test_linear_tile_cases.py).

A  every tile lands where it belongs: 16, 32 and 48 workgroups, where the XCD rotation of the tile index is not the identity (every other
   kernel test runs at most 12 workgroups, and 8 is the only multiple of 8 among them), aligned and ragged; `distinct` operands, whose
   float64 product is an fp32 number whatever the order of the sum -- a tile, row, column, slab or register taken from the wrong place
   changes the result outright.
   (768, 512, 96) is three K slabs: an odd number, which the plain loop takes on an aligned shape too.
B  rows 257 / 319 / 321 / 383 -- no multiple of 32: the C/D register map of the 32 x 32 MFMAs and the three row guards of the ragged bodies --
   with every output a view inside a larger buffer whose guard rows must keep their sentinel words.
C  a row of y, gz, dx is a function of that row's operands and w alone: the same bits for every row count (pipelined, plain and ragged
   bodies), row position, column position, and power-of-two scaling of the operands.
D  what pn_linear_fwd_form refuses: null and misaligned operands, unknown flag bits, a y that shares bytes with x, w or b."""
import pytest
import torch

import _linear_tile_cases as tc
from conftest import require_gpu

pytestmark = pytest.mark.gpu

PLAIN = 1                             # PN_LINEAR_FORM_PLAIN


def _ops():
    from pnode_amd import _lib
    from pnode_amd._vecops import HipVecOps
    assert _lib.PN_LINEAR_FORM_PLAIN == PLAIN
    return HipVecOps(require_gpu(), torch.float32, 1024 * 512)


def _forms(rows, width, k):
    """(name, flags) of the bodies a shape can take: aligned shapes the pipelined one (an even number of K slabs) and, asked for or with
    an odd number of slabs, the plain one; ragged shapes the ragged one whatever the flag."""
    if not tc.is_aligned(rows, width):
        return [("ragged", 0)]
    return [("pipelined", 0), ("plain", PLAIN)] if tc.pipelines(k) else [("plain", 0)]


def _exact(got, want64, what):
    """`got` (on the device) is the float64 result cast to fp32, bit for bit; names the tile of the first wrong element."""
    got, want = got.cpu(), want64.float()
    assert got.shape == want.shape, what
    if not torch.equal(got, want):
        tile, at, g, w, n = tc.first_wrong_tile(got, want)
        print("%s: first wrong element in tile (row // 64, col // 128) = %s at %s: got %r, want %r; %d wrong of %d" % (what, tile, at, g, w, n, want.numel()))
        pytest.fail("%s: tile %s, element %s: got %r, want %r (%d wrong)" % (what, tile, at, g, w, n))


def _same_bits(a, b, what):
    """Two results of the same rows, bit for bit; names the first element that differs and both patterns."""
    if torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32)):
        return
    bad = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    r, c = int(bad[0, 0]), int(bad[0, 1])
    pa, pb = int(a.view(torch.int32)[r, c]) & 0xFFFFFFFF, int(b.view(torch.int32)[r, c]) & 0xFFFFFFFF
    msg = "%s: %d elements differ, the first at (%d, %d): %08x against %08x (%r, %r)" % (what, bad.shape[0], r, c, pa, pb, float(a[r, c]), float(b[r, c]))
    print(msg)
    pytest.fail(msg)


# ---- A: every tile lands where it belongs, rotation included -------------------------------------------------------------------------
@pytest.mark.parametrize("rows,width,k", tc.TILE_CASES + tc.EXTRA_TILE_CASES)
def test_forward_tiles_land_where_they_belong(rows, width, k):
    ops = _ops()
    x, w, b = tc.forward_operands("distinct", rows, width, k, tc.case_seed(rows, width, k))
    want = {True: tc.forward64(x, w, b), False: tc.forward64(x, w)}
    x, w, b = (t.to(ops.device) for t in (x, w, b))
    for form, flags in _forms(rows, width, k):
        for bias in (True, False):
            y = torch.full((rows, width), float("nan"), device=ops.device)
            ops.linear_fwd(x, w, b if bias else None, False, y, flags=flags)
            _exact(y, want[bias], "forward %s, %d workgroups, %s bias" % (form, tc.workgroups(rows, width), "with" if bias else "no"))


@pytest.mark.parametrize("rows,width,k", tc.TILE_CASES + tc.EXTRA_TILE_CASES)
def test_backward_tiles_land_where_they_belong(rows, width, k):
    """gz is written by tile column 0 alone: pre-filled with NaN, it must be complete and exact with several tile columns too."""
    ops = _ops()
    g, a, w = tc.backward_operands("distinct", rows, width, k, tc.case_seed(rows, width, k))
    gz64, dx64 = tc.backward64(g, a, w)
    g, a, w = (t.to(ops.device) for t in (g, a, w))
    for form, flags in _forms(rows, width, k):
        gz = torch.full((rows, k), float("nan"), device=ops.device)
        dx = torch.full((rows, width), float("nan"), device=ops.device)
        ops.linear_bwd(g, a, w, gz, dx, flags=flags)
        what = "backward %s, %d workgroups in %d tile columns" % (form, tc.workgroups(rows, width), -(-width // tc.TILE_N))
        _exact(gz, gz64, what + ", gz")
        _exact(dx, dx64, what + ", dx")


# ---- B: ragged row counts that are no multiple of 32, and nothing outside the output --------------------------------------------------
_GUARDED = [(r, wd, k) for r in tc.RAGGED_ROWS for wd, k in tc.RAGGED_WIDTH_K] + [tc.ALIGNED_GUARD_CASE]


@pytest.mark.parametrize("rows,width,k", _GUARDED)
def test_forward_writes_its_rows_exactly_and_nothing_else(rows, width, k):
    ops = _ops()
    x, w, b = tc.forward_operands("distinct", rows, width, k, tc.case_seed(rows, width, k))
    want = {True: tc.forward64(x, w, b), False: tc.forward64(x, w)}
    x, w, b = (t.to(ops.device) for t in (x, w, b))
    for form, flags in _forms(rows, width, k):
        for bias in (True, False):
            buf, y = tc.guarded(rows, width, ops.device)
            assert y.data_ptr() % 16 == 0 and y.is_contiguous()
            ops.linear_fwd(x, w, b if bias else None, False, y, flags=flags)
            torch.cuda.synchronize()
            _exact(y, want[bias], "forward %s, rows %d" % (form, rows))
            assert tc.guards_untouched(buf, rows), "forward %s, rows %d: a store outside y" % (form, rows)


@pytest.mark.parametrize("rows,width,k", _GUARDED)
def test_backward_writes_its_rows_exactly_and_nothing_else(rows, width, k):
    ops = _ops()
    g, a, w = tc.backward_operands("distinct", rows, width, k, tc.case_seed(rows, width, k))
    gz64, dx64 = tc.backward64(g, a, w)
    g, a, w = (t.to(ops.device) for t in (g, a, w))
    for form, flags in _forms(rows, width, k):
        zbuf, gz = tc.guarded(rows, k, ops.device)
        dbuf, dx = tc.guarded(rows, width, ops.device)
        ops.linear_bwd(g, a, w, gz, dx, flags=flags)
        torch.cuda.synchronize()
        _exact(gz, gz64, "backward %s, rows %d, gz" % (form, rows))
        _exact(dx, dx64, "backward %s, rows %d, dx" % (form, rows))
        assert tc.guards_untouched(zbuf, rows), "backward %s, rows %d: a store outside gz" % (form, rows)
        assert tc.guards_untouched(dbuf, rows), "backward %s, rows %d: a store outside dx" % (form, rows)


# ---- C: a row's bits do not depend on the launch -------------------------------------------------------------------------------------
def _launches(width, k):
    """(rows, form, flags) in ascending row count: every row count, aligned ones in both forms."""
    return [(rows, form, flags) for rows in tc.ROW_COUNTS for form, flags in _forms(rows, width, k)]


def _check_row_counts(results, what):
    """results: [(rows, form, tensor)] ascending.  Every launch's first 256 rows are those of the 513-row launch, and each launch agrees
    with the next one (the next larger row count, or the other form of the same one) on all common rows."""
    rows_last, form_last, last = results[-1]
    assert rows_last == tc.MASTER_ROWS
    for rows, form, t in results:
        _same_bits(t[:256], last[:256], "%s: rows %d (%s) against rows %d (%s), first 256 rows" % (what, rows, form, rows_last, form_last))
    for (r0, f0, t0), (r1, f1, t1) in zip(results, results[1:]):
        n = min(r0, r1)
        _same_bits(t0[:n], t1[:n], "%s: rows %d (%s) against rows %d (%s), %d common rows" % (what, r0, f0, r1, f1, n))


@pytest.mark.parametrize("width,k", tc.LAUNCH_WIDTH_K + tc.EXTRA_LAUNCH_WIDTH_K)
@pytest.mark.parametrize("tanh", [False, True])
def test_forward_rows_do_not_depend_on_the_row_count(width, k, tanh):
    ops = _ops()
    x, w, b = (t.to(ops.device) for t in tc.forward_operands("normal", tc.MASTER_ROWS, width, k, 31 + width + k))
    forms = set()
    results = []
    for rows, form, flags in _launches(width, k):
        results.append((rows, form, ops.linear_fwd(x[:rows], w, b, tanh, flags=flags)))
        forms.add(form)
    assert "ragged" in forms and (width % tc.TILE_N or "plain" in forms) and (width % tc.TILE_N or not tc.pipelines(k) or "pipelined" in forms)
    _check_row_counts(results, "forward y (tanh %s, width %d, K %d)" % (tanh, width, k))


@pytest.mark.parametrize("width,k", tc.LAUNCH_WIDTH_K + tc.EXTRA_LAUNCH_WIDTH_K)
def test_backward_rows_do_not_depend_on_the_row_count(width, k):
    ops = _ops()
    g, a, w = (t.to(ops.device) for t in tc.backward_operands("normal", tc.MASTER_ROWS, width, k, 47 + width + k))
    gzs, dxs = [], []
    for rows, form, flags in _launches(width, k):
        gz, dx = ops.linear_bwd(g[:rows], a[:rows], w, flags=flags)
        gzs.append((rows, form, gz))
        dxs.append((rows, form, dx))
    _check_row_counts(gzs, "backward gz (width %d, K %d)" % (width, k))
    _check_row_counts(dxs, "backward dx (width %d, K %d)" % (width, k))


@pytest.mark.parametrize("width,k", tc.LAUNCH_WIDTH_K)
@pytest.mark.parametrize("rows", tc.ROLL_ROW_COUNTS)
def test_rows_do_not_depend_on_their_position(rows, width, k):
    ops = _ops()
    s = tc.ROW_ROLL
    x, w, b = (t.to(ops.device) for t in tc.forward_operands("normal", rows, width, k, 5 + rows + width))
    g, a, wb = (t.to(ops.device) for t in tc.backward_operands("normal", rows, width, k, 6 + rows + width))
    for form, flags in _forms(rows, width, k):
        for tanh in (False, True):
            y = ops.linear_fwd(x, w, b, tanh, flags=flags)
            yr = ops.linear_fwd(x.roll(s, 0).contiguous(), w, b, tanh, flags=flags)
            _same_bits(yr, y.roll(s, 0), "forward %s (tanh %s): rows rolled by %d" % (form, tanh, s))
        gz, dx = ops.linear_bwd(g, a, wb, flags=flags)
        gzr, dxr = ops.linear_bwd(g.roll(s, 0).contiguous(), a.roll(s, 0).contiguous(), wb, flags=flags)
        _same_bits(gzr, gz.roll(s, 0), "backward %s: gz, rows rolled by %d" % (form, s))
        _same_bits(dxr, dx.roll(s, 0), "backward %s: dx, rows rolled by %d" % (form, s))


@pytest.mark.parametrize("width,k", tc.LAUNCH_WIDTH_K)
@pytest.mark.parametrize("rows", [384, 257])
def test_columns_do_not_depend_on_their_position(rows, width, k):
    """Rolling the rows of w (forward: with the bias) or the columns of w (backward) by 45 rolls the columns of y / dx: a column moves to
    another lane, another accumulator, another K half's epilogue and, at width 192, another tile column."""
    ops = _ops()
    s = tc.COL_ROLL
    x, w, b = (t.to(ops.device) for t in tc.forward_operands("normal", rows, width, k, 7 + rows + width))
    g, a, wb = (t.to(ops.device) for t in tc.backward_operands("normal", rows, width, k, 8 + rows + width))
    for form, flags in _forms(rows, width, k):
        for tanh in (False, True):
            y = ops.linear_fwd(x, w, b, tanh, flags=flags)
            yr = ops.linear_fwd(x, w.roll(s, 0).contiguous(), b.roll(s, 0).contiguous(), tanh, flags=flags)
            _same_bits(yr, y.roll(s, 1), "forward %s (tanh %s): columns rolled by %d" % (form, tanh, s))
        gz, dx = ops.linear_bwd(g, a, wb, flags=flags)
        gzr, dxr = ops.linear_bwd(g, a, wb.roll(s, 1).contiguous(), flags=flags)
        _same_bits(gzr, gz, "backward %s: gz, columns of w rolled" % form)
        _same_bits(dxr, dx.roll(s, 1), "backward %s: dx, columns rolled by %d" % (form, s))


@pytest.mark.parametrize("rows,width,k", tc.SCALING_CASES)
def test_powers_of_two_scale_the_product_exactly(rows, width, k):
    """linear_fwd(2^p x, 2^q w) == 2^(p + q) linear_fwd(x, w) bit for bit (identity, no bias), and dx likewise with g and w scaled: no term
    of the split or of the six products is subnormal or overflows at these exponents (tests/test_linear_tile_cases.py), so every rounding
    happens at the same bit -- all three bf16 parts at exponents far from 1."""
    ops = _ops()
    seed = tc.case_seed(rows, width, k)
    x, w, _ = (t.to(ops.device) for t in tc.forward_operands("normal", rows, width, k, seed))
    g, a, wb = (t.to(ops.device) for t in tc.backward_operands("normal", rows, width, k, seed))
    for form, flags in _forms(rows, width, k):
        y = ops.linear_fwd(x, w, None, False, flags=flags)
        gz, dx = ops.linear_bwd(g, a, wb, flags=flags)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
        for p, q in tc.SCALINGS:
            ys = ops.linear_fwd(x * 2.0 ** p, w * 2.0 ** q, None, False, flags=flags)
            _same_bits(ys, y * 2.0 ** (p + q), "forward %s: x 2^%d, w 2^%d" % (form, p, q))
            gzs, dxs = ops.linear_bwd(g * 2.0 ** p, a, wb * 2.0 ** q, flags=flags)
            _same_bits(gzs, gz * 2.0 ** p, "backward %s: gz, g 2^%d" % (form, p))
            _same_bits(dxs, dx * 2.0 ** (p + q), "backward %s: dx, g 2^%d, w 2^%d" % (form, p, q))


# ---- D: the forward's refusals -------------------------------------------------------------------------------------------------------
def _off16(t):
    """A contiguous copy of t that starts at element 1 of a larger buffer: 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 4, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _fwd_case(ops, rows=256, width=128, k=64):
    x, w, b = (t.to(ops.device) for t in tc.forward_operands("normal", rows, width, k, 77))
    return x, w, b, torch.full((rows, width), 7.0, device=ops.device)


def _is7(y):
    torch.cuda.synchronize()
    return bool((y == 7.0).all())


def test_null_operands_are_refused_and_nothing_is_launched():
    from pnode_amd import _lib
    ops = _ops()
    rows, width, k = 256, 128, 64
    x, w, b, y = _fwd_case(ops, rows, width, k)
    lib, st, code = _lib.load(), ops.stream(), _lib.dtype_code(torch.float32)
    ptrs = {"x": x.data_ptr(), "w": w.data_ptr(), "y": y.data_ptr()}
    for null in ("x", "w", "y"):
        p = dict(ptrs)
        p[null] = None
        for flags in (0, PLAIN):
            assert lib.pn_linear_fwd_form(st, code, rows, width, k, p["x"], p["w"], b.data_ptr(), _lib.PN_ACT_IDENTITY, p["y"], flags) != 0, null
        assert lib.pn_linear_fwd(st, code, rows, width, k, p["x"], p["w"], b.data_ptr(), _lib.PN_ACT_TANH, p["y"]) != 0, null
        assert "null" in lib.pn_last_error().decode()
        assert _is7(y)
    # all of them there (a null bias is no bias): launched
    assert lib.pn_linear_fwd_form(st, code, rows, width, k, ptrs["x"], ptrs["w"], None, _lib.PN_ACT_IDENTITY, ptrs["y"], 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, ops.linear_fwd(x, w, None, False))


@pytest.mark.parametrize("rows,width", [(256, 128), (257, 192)])
def test_misaligned_operands_are_refused_and_a_misaligned_bias_is_not(rows, width):
    from pnode_amd._lib import PnError
    ops = _ops()
    k = 64
    x, w, b, y = _fwd_case(ops, rows, width, k)
    for form, flags in _forms(rows, width, k):
        for args in ((_off16(x), w, b, False, y), (x, _off16(w), b, False, y)):
            with pytest.raises(PnError, match="aligned"):
                ops.linear_fwd(*args, flags=flags)
            assert _is7(y)
        y1 = _off16(y)
        with pytest.raises(PnError, match="aligned"):
            ops.linear_fwd(x, w, b, False, y1, flags=flags)
        assert _is7(y1) and _is7(y)
        # the bias is read one value at a time: 4-byte alignment is enough, and the bits are those of an aligned bias
        b1 = _off16(b)
        for tanh in (False, True):
            _same_bits(ops.linear_fwd(x, w, b1, tanh, flags=flags), ops.linear_fwd(x, w, b, tanh, flags=flags), "%s: a bias at 4 bytes off" % form)


def test_unknown_flag_bits_are_refused_forward_and_backward():
    from pnode_amd._lib import PnError
    ops = _ops()
    rows, width, k = 256, 128, 64
    x, w, b, y = _fwd_case(ops, rows, width, k)
    g, a, wb = (t.to(ops.device) for t in tc.backward_operands("normal", rows, width, k, 78))
    gz, dx = torch.full((rows, k), 7.0, device=ops.device), torch.full((rows, width), 7.0, device=ops.device)
    for flags in (2, 2 | PLAIN, 4, 1 << 30, -1):
        with pytest.raises(PnError, match="flag"):
            ops.linear_fwd(x, w, b, True, y, flags=flags)
        with pytest.raises(PnError, match="flag"):
            ops.linear_bwd(g, a, wb, gz, dx, flags=flags)
        assert _is7(y) and _is7(gz) and _is7(dx)


def _refused_unchanged(ops, pool, x, w, b, y, what):
    from pnode_amd._lib import PnError
    before = pool.clone()
    for flags in (0, PLAIN):
        with pytest.raises(PnError, match="alias"):
            ops.linear_fwd(x, w, b, False, y, flags=flags)
    torch.cuda.synchronize()
    assert torch.equal(pool, before), what


@pytest.mark.parametrize("rows,width,k", [(256, 128, 64), (257, 64, 64)])
def test_a_y_that_shares_bytes_with_an_input_is_refused(rows, width, k):
    """Identity, and partial overlaps of 16 bytes at either end of x, w and b; y touching an input without sharing a byte goes through."""
    ops = _ops()
    x0, w0, b0 = (t.to(ops.device) for t in tc.forward_operands("normal", rows, width, k, 79))
    nx, nw, ny, nb = rows * k, width * k, rows * width, width

    def pool():
        """room for y | the operand under test | room for y | the other two operands"""
        return torch.full((2 * ny + nx + nw + nb,), 7.0, device=ops.device)

    def at(p, start, n, shape):
        assert start % 4 == 0
        return p[start:start + n].view(shape)

    # y over the tail of x, over the head of x, and (where the shapes allow it) x itself
    p = pool()
    x, w, b = at(p, ny, nx, (rows, k)), at(p, ny + nx + ny, nw, (width, k)), at(p, ny + nx + ny + nw, nb, (nb,))
    x.copy_(x0), w.copy_(w0), b.copy_(b0)
    _refused_unchanged(ops, p, x, w, b, at(p, ny + nx - 4, ny, (rows, width)), "y begins in the last 16 bytes of x")
    _refused_unchanged(ops, p, x, w, b, at(p, 4, ny, (rows, width)), "y ends in the first 16 bytes of x")
    if k == width:
        _refused_unchanged(ops, p, x, w, b, x, "y is x")
    # y touching x on either side shares no byte with it: launched, and right
    want = ops.linear_fwd(x0, w0, b0, False)
    y = at(p, 0, ny, (rows, width))
    ops.linear_fwd(x, w, b, False, y)
    _same_bits(y, want, "y ends where x begins")
    y = at(p, ny + nx, ny, (rows, width))             # between x and w, touching both
    ops.linear_fwd(x, w, b, False, y)
    _same_bits(y, want, "y between x and w")
    # w: y begins in its last 16 bytes; y ends in its first 16 bytes; w inside y
    p = pool()
    w, x, b = at(p, ny, nw, (width, k)), at(p, ny + nw + ny, nx, (rows, k)), at(p, ny + nw + ny + nx, nb, (nb,))
    x.copy_(x0), w.copy_(w0), b.copy_(b0)
    _refused_unchanged(ops, p, x, w, b, at(p, ny + nw - 4, ny, (rows, width)), "y begins in the last 16 bytes of w")
    _refused_unchanged(ops, p, x, w, b, at(p, 4, ny, (rows, width)), "y ends in the first 16 bytes of w")
    _refused_unchanged(ops, p, x, w, b, at(p, ny - 4, ny, (rows, width)), "w inside y")
    assert ny - 4 >= nw
    y = at(p, ny + nw, ny, (rows, width))             # between w and x, touching both
    ops.linear_fwd(x, w, b, False, y)
    _same_bits(y, want, "y between w and x")
    # b: y begins in its last 16 bytes; y ends in its first 16 bytes; b inside y
    p = pool()
    b, x, w = at(p, ny, nb, (nb,)), at(p, ny + nb + ny, nx, (rows, k)), at(p, ny + nb + ny + nx, nw, (width, k))
    x.copy_(x0), w.copy_(w0), b.copy_(b0)
    _refused_unchanged(ops, p, x, w, b, at(p, ny + nb - 4, ny, (rows, width)), "y begins in the last 16 bytes of b")
    _refused_unchanged(ops, p, x, w, b, at(p, 4, ny, (rows, width)), "y ends in the first 16 bytes of b")
    _refused_unchanged(ops, p, x, w, b, at(p, ny - 128, ny, (rows, width)), "b inside y")
    y = at(p, ny + nb, ny, (rows, width))             # between b and x, touching both
    ops.linear_fwd(x, w, b, False, y)
    _same_bits(y, want, "y between b and x")
    # last (it overwrites b): the y that covers b, without a bias, shares nothing the launch reads
    y = at(p, ny - 128, ny, (rows, width))
    ops.linear_fwd(x, w, None, False, y)
    _same_bits(y, ops.linear_fwd(x0, w0, None, False), "no bias: the bytes of b are not read")


# ---- an odd number of K slabs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,width,k", [(256, 128, 96), (257, 192, 96), (384, 256, 160)])
def test_an_odd_number_of_slabs_is_as_close_to_float64_as_the_library(rows, width, k):
    """K = 96 / 160 (three / five slabs) on random operands, by the bars of tests/test_gpu_linear_fwd.py (2 x the library path's own error
    from float64, in units of sum |x w| + |b|) and tests/test_gpu_linear_bwd.py (gz within 3 * 2^-24 |g|; dx 1.5 x the library's error)."""
    import torch.nn.functional as F
    ops = _ops()
    assert ops.linear_fwd_supported(rows, width, k) and ops.linear_bwd_supported(rows, k, width)
    x, w, b = (t.to(ops.device) for t in tc.forward_operands("normal", rows, width, k, 91 + k))
    for tanh in (False, True):
        act = torch.tanh if tanh else (lambda t: t)
        y = ops.linear_fwd(x, w, b, tanh)
        _same_bits(y, ops.linear_fwd(x, w, b, tanh, flags=PLAIN), "forward, tanh %s: the flag changes nothing" % tanh)
        z64 = tc.forward64(x, w, b)
        scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
        e_lib = float(((act(F.linear(x, w, b)).double() - act(z64)).abs() / scale).max())
        e_own = float(((y.double() - act(z64)).abs() / scale).max())
        print("forward K %d tanh %s: pn_linear_fwd %.3e  library %.3e" % (k, tanh, e_own, e_lib))
        assert e_own <= 2.0 * e_lib
    g, a, wb = (t.to(ops.device) for t in tc.backward_operands("normal", rows, width, k, 92 + k))
    gz, dx = ops.linear_bwd(g, a, wb)
    assert bool(((gz.double() - tc.gz64(g, a)).abs() <= 3.0 * 2.0 ** -24 * g.double().abs()).all())
    dx64, scale = gz.double() @ wb.double(), gz.double().abs() @ wb.double().abs()
    e_lib = float(((torch.matmul(gz, wb).double() - dx64).abs() / scale).max())
    e_own = float(((dx.double() - dx64).abs() / scale).max())
    print("backward K %d: pn_linear_bwd %.3e  library %.3e" % (k, e_own, e_lib))
    assert e_own <= 1.5 * e_lib
