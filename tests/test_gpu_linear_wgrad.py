"""-m gpu: pn_linear_wgrad_group / pn_linear_wgrad_finish (csrc/pn_linear.hip) pinned with exact operands, through HipVecOps.  Everything
compares bits or exact values -- there is no tolerance in this file; operands, references and premises are tests/_wgrad_cases.py (checked on
the CPU by tests/test_wgrad_cases.py).  Every group runs the four 64 x 64 forms (split-bf16 by default and under PN_WGRAD_TILE_64,
PN_WGRAD_EXACT_FP32, fp64), each in its aligned and its ragged instantiation as the row count decides, and the 128 x 128 form on a group of
two 512 x 512 pairs, which the launcher takes by its own rule (computed here from the device's CU count; skipped with a message if the
device is not one on which that group fills whole rounds).

A  tiles, K ranges and slabs land where they belong: `distinct` operands, accumulating launches that never cancel; pw and pb against float64 in their own
   layout, before the finish; then mu exact, the partials zero, mu_b untouched without pb.
B  the same with pw, pb, mu_w and mu_b inside guards of sentinel words (mu_b off the 16-byte boundary): nothing outside the buffers.
C  one product per element of dW: each of the six products of the split shows in the bits; a subnormal bf16 part.
D  power-of-two scaling of G and X scales pw and pb exactly; rolling the rows by whole K ranges permutes the ranges and leaves their bits.
E  a NaN or an infinity in G or X reaches its own row or column of its own K range, and its own slot of pb, and nothing else.
F  groups of 1, 4, 8 and 10 pairs of mixed shapes, a power-of-two alpha each: every pair's partials exact."""
import pytest
import torch

import _linear_tile_cases as tc
import _wgrad_cases as wc
from conftest import require_gpu

pytestmark = pytest.mark.gpu

WIDE = "wide"


def _ops(dtype, flags):
    from pnode_amd import _lib
    from pnode_amd._vecops import HipVecOps
    assert (_lib.PN_WGRAD_EXACT_FP32, _lib.PN_WGRAD_TILE_64, _lib.PN_WGRAD_MAX_PAIRS) == (wc.EXACT_FP32, wc.TILE_64, 8)
    ops = HipVecOps(require_gpu(), dtype, 64)
    ops.wgrad_flags = flags
    return ops


def _wide_ops():
    """HipVecOps with flags 0 on a device where the wide group takes the 128 x 128 form -- never silently the 64 x 64 one."""
    ops = _ops(torch.float32, 0)
    cus = torch.cuda.get_device_properties(ops.device).multi_processor_count
    if not wc.takes_wide(wc.WIDE_GROUP, cus):
        pytest.skip("%d CUs: a group of %r does not take the 128 x 128 form here" % (cus, wc.WIDE_GROUP))
    return ops


def _forms(wide):
    """(name, ops) of the forms a case runs: the wide group under flags 0 and, for contrast, PN_WGRAD_TILE_64; else the four 64 x 64 forms."""
    if wide:
        return [(WIDE, _wide_ops()), ("wide group, 64 x 64 tiles", _ops(torch.float32, wc.TILE_64))]
    return [(name, _ops(dtype, flags)) for name, dtype, flags in wc.FORMS]


def _fp32_forms(wide):
    return [(name, ops) for name, ops in _forms(wide) if ops.dtype == torch.float32]


def _dev(ops, *ts):
    return tuple(t.to(ops.dtype).to(ops.device) for t in ts)


def _launch(ops, layers, alphas, bufs):
    """One grouped launch (two beyond eight pairs): layers [(G, X)] on the device, an alpha and a (pw, pb) each."""
    ops.linear_wgrad_group([(G, X, a, pw, pb) for (G, X), a, (pw, pb) in zip(layers, alphas, bufs)])


def _buffers(ops, layers, biases):
    return [ops.linear_wgrad_buffers(G.shape[1], X.shape[1], b) for (G, X), b in zip(layers, biases)]


def _exact_pw(pw, want64, dtype, what):
    """The flat pw is the float64 reference (8, out_f, in_f) cast to the state's dtype, bit for bit; names range, tile and element."""
    want = want64.to(dtype)
    got = pw.view(want.shape).cpu()
    if not torch.equal(got, want):
        s, tile, at, g, w, n = wc.first_wrong(got, want)
        pytest.fail("%s: pw, K range %d, tile (m // 64, n // 64) = %s, element %s: got %r, want %r (%d wrong of %d)" % (what, s, tile, at, g, w, n, want.numel()))


def _exact_pb(pb, want64, what):
    got = pb.view(want64.shape).cpu()
    assert got.dtype == torch.float64
    if not torch.equal(got, want64):
        bad = (got != want64).nonzero()
        s, j, m = (int(v) for v in bad[0])
        pytest.fail("%s: pb, K range %d, tile column %d, column %d of G: got %r, want %r (%d wrong of %d)" % (
            what, s, j, m, float(got[s, j, m]), float(want64[s, j, m]), bad.shape[0], want64.numel()))


def _exact_mu(got, want64, what):
    want = want64.to(got.dtype)
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        at = tuple(int(v) for v in bad[0])
        pytest.fail("%s: element %s: got %r, want %r (%d wrong)" % (what, at, float(got[at]), float(want[at]), bad.shape[0]))


def _same_bits(a, b, what):
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    else:
        a, b = a.view(torch.int32), b.view(torch.int32)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        at = tuple(int(v) for v in bad[0])
        pytest.fail("%s: %d elements differ, the first at %s: %x against %x" % (what, bad.shape[0], at, int(a[at]) & (2 ** 64 - 1), int(b[at]) & (2 ** 64 - 1)))


def _check_finish(ops, layer, buf, mu, start, want, bias, what):
    """pn_linear_wgrad_finish of one pair: mu exact, the partials zero, mu_b untouched when there is no pb."""
    (G, X), (pw, pb), (mu_w, mu_b), (w0, b0), (pw64, pb64) = layer, buf, mu, start, want
    ops.linear_wgrad_finish(G.shape[1], X.shape[1], pw, pb, mu_w, mu_b)
    torch.cuda.synchronize()
    _exact_mu(mu_w, w0.double() + pw64.sum(0), what + ", mu_w")
    if bias:
        _exact_mu(mu_b, b0.double() + pb64.sum((0, 1)), what + ", mu_b")
        assert not bool(pb.any()), what + ": pb is not zero after the finish"
    else:
        _exact_mu(mu_b, b0.double(), what + ", mu_b without pb")
    assert not bool(pw.any()), what + ": pw is not zero after the finish"


# ---- A: tiles, K ranges and slabs land where they belong ------------------------------------------------------------------------------
def _run_exact(rows, shapes, wide):
    alphas = wc.alphas_for(rows)
    cpu = wc.exact_layers(rows, shapes)
    refs = {}
    for name, ops in _forms(wide):
        if ops.dtype not in refs:
            refs[ops.dtype] = [wc.accumulated64(G, X, alphas, ops.dtype) for G, X in cpu]
        want = refs[ops.dtype]
        assert all(bool(pw64[s].any()) for pw64, _ in want for s in range(8) if s * wc.kper(rows) < rows)      # nothing cancels
        layers = [_dev(ops, G, X) for G, X in cpu]
        for bias in (True, False):
            what = "%s, rows %d (%s), %s" % (name, rows, "ragged" if wc.is_ragged(rows) else "aligned", "bias" if bias else "no bias")
            bufs = _buffers(ops, layers, [bias] * len(layers))
            for a in alphas:
                _launch(ops, layers, [a] * len(layers), bufs)
            torch.cuda.synchronize()
            for k, ((pw, pb), (pw64, pb64)) in enumerate(zip(bufs, want)):
                _exact_pw(pw, pw64, ops.dtype, "%s, pair %d %r" % (what, k, shapes[k]))
                if bias:
                    _exact_pb(pb, pb64, "%s, pair %d %r" % (what, k, shapes[k]))
            for k, (layer, buf, w64) in enumerate(zip(layers, bufs, want)):
                start = wc.mu_start(shapes[k][0], shapes[k][1], wc.seed_of(rows, *shapes[k]))
                mu = tuple(t.clone() for t in _dev(ops, *start))
                _check_finish(ops, layer, buf, mu, start, w64, bias, "%s, pair %d, finish" % (what, k))


@pytest.mark.parametrize("rows,out_f,in_f", wc.A_CASES)
def test_partials_land_in_their_ranges_tiles_and_slots(rows, out_f, in_f):
    _run_exact(rows, [(out_f, in_f)], False)


@pytest.mark.parametrize("rows", wc.A_WIDE_ROWS)
def test_partials_of_the_wide_form_land_in_the_slots_of_the_64_form(rows):
    """Both runs against the same float64 layout: the 128 x 128 form fills the slots 2 tn and 2 tn + 1 of the 64-wide tile columns."""
    _run_exact(rows, wc.WIDE_GROUP, True)


# ---- B: nothing outside the buffers ------------------------------------------------------------------------------------------------
def _run_guarded(rows, shapes, wide):
    alphas = wc.alphas_for(rows)
    cpu = wc.exact_layers(rows, shapes)
    for name, ops in _forms(wide):
        want = [wc.accumulated64(G, X, alphas, ops.dtype) for G, X in cpu]
        layers = [_dev(ops, G, X) for G, X in cpu]
        what = "%s, rows %d" % (name, rows)
        guards, bufs, mus, starts = [], [], [], []
        for k, (o, i) in enumerate(shapes):
            ntn = i // wc.BN
            g_pw = wc.guarded_flat(8 * o * i, o * i, ops.dtype, ops.device)                   # a whole partial plane either side
            g_pb = wc.guarded_flat(8 * ntn * o, ntn * o, torch.float64, ops.device)           # a K range's slots either side
            g_mw = wc.guarded_flat(o * i, 64 * i, ops.dtype, ops.device)                      # a tile row either side
            g_mb = wc.guarded_flat(o, 64, ops.dtype, ops.device, skew=1)                      # and not 16-byte aligned
            assert g_pw[1].data_ptr() % 16 == 0 and g_mw[1].data_ptr() % 16 == 0 and g_mb[1].data_ptr() % 16 != 0
            g_pw[1].zero_(), g_pb[1].zero_()
            start = wc.mu_start(o, i, wc.seed_of(rows, o, i))
            g_mw[1].copy_(start[0].reshape(-1)), g_mb[1].copy_(start[1])
            guards.append((g_pw, g_pb, g_mw, g_mb))
            bufs.append((g_pw[1], g_pb[1]))
            mus.append((g_mw[1].view(o, i), g_mb[1]))
            starts.append(start)

        def untouched(when):
            torch.cuda.synchronize()
            for k, gs in enumerate(guards):
                for label, (words, _, span) in zip(("pw", "pb", "mu_w", "mu_b"), gs):
                    assert wc.guards_ok(words, span), "%s, pair %d, %s: a store outside %s" % (what, k, when, label)
        for n, a in enumerate(alphas):
            _launch(ops, layers, [a] * len(layers), bufs)
            untouched("launch %d" % n)
        for k, ((pw, pb), (pw64, pb64)) in enumerate(zip(bufs, want)):
            _exact_pw(pw, pw64, ops.dtype, "%s, pair %d" % (what, k))
            _exact_pb(pb, pb64, "%s, pair %d" % (what, k))
        for k, (layer, buf, mu, start, w64) in enumerate(zip(layers, bufs, mus, starts, want)):
            _check_finish(ops, layer, buf, mu, start, w64, True, "%s, pair %d, finish" % (what, k))
        untouched("finish")


@pytest.mark.parametrize("rows,out_f,in_f", wc.B_CASES)
def test_launches_and_finish_write_their_buffers_and_nothing_else(rows, out_f, in_f):
    _run_guarded(rows, [(out_f, in_f)], False)


@pytest.mark.parametrize("rows", wc.B_WIDE_ROWS)
def test_the_wide_form_writes_its_buffers_and_nothing_else(rows):
    _run_guarded(rows, wc.WIDE_GROUP, True)


# ---- C: the six products of the split, one product per element --------------------------------------------------------------------------
def _run_impulses(kind, rows, shapes, wide):
    cpu = [wc.impulse_operands(kind, rows, o, i, wc.pair_seed(rows, o, i, k)) for k, (o, i) in enumerate(shapes)]
    alpha, bias = cpu[0][2], cpu[0][3]
    for name, ops in _forms(wide):
        want = [wc.partials64(G, X, alpha, ops.dtype) for G, X, _, _ in cpu]
        assert all(wc.is_exact_in(pw64, ops.dtype) for pw64, _ in want)
        layers = [_dev(ops, G, X) for G, X, _, _ in cpu]
        bufs = _buffers(ops, layers, [bias] * len(layers))
        _launch(ops, layers, [alpha] * len(layers), bufs)
        torch.cuda.synchronize()
        for k, ((pw, pb), (pw64, pb64)) in enumerate(zip(bufs, want)):
            what = "%s, %s, rows %d, pair %d %r" % (name, kind, rows, k, shapes[k])
            _exact_pw(pw, pw64, ops.dtype, what)
            if bias:
                _exact_pb(pb, pb64, what)


@pytest.mark.parametrize("kind,rows,out_f,in_f", wc.C_CASES)
def test_each_product_of_the_split_arrives(kind, rows, out_f, in_f):
    _run_impulses(kind, rows, [(out_f, in_f)], False)


@pytest.mark.parametrize("kind,rows", wc.C_WIDE_CASES)
def test_each_product_of_the_split_arrives_in_the_wide_form(kind, rows):
    _run_impulses(kind, rows, wc.WIDE_GROUP, True)


# ---- D: power-of-two scaling and row position give the same bits -----------------------------------------------------------------------
def _normal_layers(ops, rows, shapes):
    return [_dev(ops, *wc.normal_operands(rows, o, i, wc.seed_of(rows, o, i) + k)) for k, (o, i) in enumerate(shapes)]


def _partials(ops, layers, alpha=1.0):
    bufs = _buffers(ops, layers, [True] * len(layers))
    _launch(ops, layers, [alpha] * len(layers), bufs)
    return bufs


def _run_scalings(rows, shapes, wide):
    for name, ops in _fp32_forms(wide):
        layers = _normal_layers(ops, rows, shapes)
        base = _partials(ops, layers)
        assert all(bool(torch.isfinite(pw).all()) and bool(pw.any()) for pw, _ in base)
        for p, q in tc.SCALINGS:
            scaled = _partials(ops, [(G * 2.0 ** p, X * 2.0 ** q) for G, X in layers])
            for k, ((pw, pb), (pws, pbs)) in enumerate(zip(base, scaled)):
                what = "%s, rows %d, pair %d: G 2^%d, X 2^%d" % (name, rows, k, p, q)
                _same_bits(pws, pw * 2.0 ** (p + q), what + ", pw")
                _same_bits(pbs, pb * 2.0 ** p, what + ", pb")


@pytest.mark.parametrize("rows,out_f,in_f", wc.SCALING_CASES)
def test_powers_of_two_scale_the_partials_exactly(rows, out_f, in_f):
    _run_scalings(rows, [(out_f, in_f)], False)


@pytest.mark.parametrize("rows", wc.SCALING_WIDE_ROWS)
def test_powers_of_two_scale_the_partials_of_the_wide_form_exactly(rows):
    _run_scalings(rows, wc.WIDE_GROUP, True)


def _run_rolls(rows, shapes, wide):
    shift = wc.ROLL_RANGES * wc.kper(rows)
    for name, ops in _forms(wide):
        layers = _normal_layers(ops, rows, shapes)
        base = _partials(ops, layers)
        rolled = _partials(ops, [(G.roll(shift, 0).contiguous(), X.roll(shift, 0).contiguous()) for G, X in layers])
        for k, ((pw, pb), (pwr, pbr), (o, i)) in enumerate(zip(base, rolled, shapes)):
            what = "%s, rows %d, pair %d: rows rolled by %d K ranges" % (name, rows, k, wc.ROLL_RANGES)
            _same_bits(pwr.view(8, o, i), pw.view(8, o, i).roll(wc.ROLL_RANGES, 0), what + ", pw")
            _same_bits(pbr.view(8, -1, o), pb.view(8, -1, o).roll(wc.ROLL_RANGES, 0), what + ", pb")
            assert not torch.equal(pwr, pw)


@pytest.mark.parametrize("rows,out_f,in_f", wc.ROLL_CASES)
def test_a_k_range_does_not_depend_on_its_position(rows, out_f, in_f):
    _run_rolls(rows, [(out_f, in_f)], False)


@pytest.mark.parametrize("rows", wc.ROLL_WIDE_ROWS)
def test_a_k_range_of_the_wide_form_does_not_depend_on_its_position(rows):
    _run_rolls(rows, wc.WIDE_GROUP, True)


# ---- E: non-finite operands keep to themselves --------------------------------------------------------------------------------------
_POISON = {"nan-g": float("nan"), "nan-x": float("nan"), "+inf-g": float("inf"), "-inf-g": float("-inf")}


def _finish_all(ops, layers, bufs, shapes, rows):
    mus = []
    for (G, X), (pw, pb), (o, i) in zip(layers, bufs, shapes):
        mu_w, mu_b = (t.clone() for t in _dev(ops, *wc.mu_start(o, i, wc.seed_of(rows, o, i))))
        ops.linear_wgrad_finish(o, i, pw, pb, mu_w, mu_b)
        mus.append((mu_w, mu_b))
    return mus


def _only_there(got, clean, mask, what):
    """Outside `mask` the bits of the clean run; the non-finite elements are exactly those of `mask`."""
    mask = mask.to(got.device).view(got.shape)
    nonfinite = ~torch.isfinite(got)
    if not torch.equal(nonfinite, mask):
        bad = (nonfinite != mask).nonzero()
        pytest.fail("%s: %d non-finite elements, %d expected; the first difference at %s" % (what, int(nonfinite.sum()), int(mask.sum()), tuple(int(v) for v in bad[0])))
    _same_bits(torch.where(mask, torch.zeros_like(got), got), torch.where(mask, torch.zeros_like(clean), clean), what + ", outside the poisoned set")


def _run_poisons(rows, shapes, places, wide):
    o, i = shapes[0]
    for name, ops in _forms(wide):
        split = ops.dtype == torch.float32 and not (ops.wgrad_flags & wc.EXACT_FP32)
        layers = _normal_layers(ops, rows, shapes)
        clean = _partials(ops, layers)
        clean = [(pw.clone(), pb.clone()) for pw, pb in clean]
        clean_mu = _finish_all(ops, layers, [(pw.clone(), pb.clone()) for pw, pb in clean], shapes, rows)
        assert all(bool(torch.isfinite(pw).all()) and bool(torch.isfinite(pb).all()) for pw, pb in clean)
        for k0, m0, n0 in places:
            for kind in wc.POISONS:
                what = "%s, rows %d, %s at row %d (range, slab, half %r), column %d" % (name, rows, kind, k0, wc.place_of(rows, k0), n0 if kind == "nan-x" else m0)
                G, X = (t.clone() for t in layers[0])
                if kind == "nan-x":
                    X[k0, n0] = _POISON[kind]
                else:
                    G[k0, m0] = _POISON[kind]
                bufs = _partials(ops, [(G, X)] + layers[1:])
                mw, mb = wc.poisoned_masks(kind, rows, o, i, k0, m0, n0)
                pw, pb = bufs[0]
                _only_there(pw, clean[0][0], mw, what + ", pw")
                _only_there(pb, clean[0][1], mb, what + ", pb")
                hit_w, hit_b = pw[mw.view(-1).to(ops.device)], pb[mb.view(-1).to(ops.device)]
                if kind.startswith("nan") or split:                # NaN stays NaN; the split turns an infinity into NaN (inf - inf)
                    assert bool(torch.isnan(hit_w).all()), what + ": pw is not NaN there"
                if kind.startswith("nan"):
                    assert bool(torch.isnan(hit_b).all()), what
                else:                                              # the column sums take the unsplit values: +-inf on every form
                    assert hit_b.tolist() == [_POISON[kind]], what + ": the slot of pb is %r" % hit_b.tolist()
                for pair in range(1, len(layers)):                 # the other pairs of the group: the clean bits
                    _same_bits(bufs[pair][0], clean[pair][0], what + ", pw of pair %d" % pair)
                    _same_bits(bufs[pair][1], clean[pair][1], what + ", pb of pair %d" % pair)
                mus = _finish_all(ops, [(G, X)] + layers[1:], bufs, shapes, rows)
                _only_there(mus[0][0], clean_mu[0][0], mw.any(0), what + ", mu_w")
                _only_there(mus[0][1], clean_mu[0][1], mb.any(0).any(0), what + ", mu_b")
                if kind.startswith("nan"):
                    assert int(torch.isnan(mus[0][0]).sum()) == int(mw.any(0).sum()) and int(torch.isnan(mus[0][1]).sum()) == int(mb.any(0).any(0).sum()), what
                for pair in range(1, len(layers)):
                    _same_bits(mus[pair][0], clean_mu[pair][0], what + ", mu_w of pair %d" % pair)


@pytest.mark.parametrize("rows,out_f,in_f,places", wc.E_CASES)
def test_a_non_finite_operand_stays_in_its_row_or_column(rows, out_f, in_f, places):
    _run_poisons(rows, [(out_f, in_f)], places, False)


@pytest.mark.parametrize("rows,places", wc.E_WIDE_CASES)
def test_a_non_finite_operand_stays_in_its_row_or_column_in_the_wide_form(rows, places):
    _run_poisons(rows, wc.WIDE_GROUP, places, True)


# ---- F: groups, exactly ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", wc.F_COUNTS)
@pytest.mark.parametrize("rows", wc.F_ROWS)
def test_every_pair_of_a_group_is_exact(rows, count):
    """The `first[]` lookup and the per-pair M, N and alpha of a grouped launch against float64: pairs of mixed shapes, with and without
    bias, a different power-of-two alpha each, two accumulating launches (alpha, then -2 alpha); ten pairs go as two launches of 8 + 2."""
    shapes = wc.F_SHAPES[:count]
    cpu = [wc.exact_operands(rows, o, i, wc.seed_of(rows, o, i) + k) for k, (o, i, _) in enumerate(shapes)]
    for name, ops in _forms(False):
        layers = [_dev(ops, G, X) for G, X in cpu]
        bufs = _buffers(ops, layers, [b for _, _, b in shapes])
        for factor in (1.0, -2.0):
            _launch(ops, layers, [factor * wc.f_alpha(k) for k in range(count)], bufs)
        torch.cuda.synchronize()
        for k, ((G, X), (pw, pb), (o, i, bias)) in enumerate(zip(cpu, bufs, shapes)):
            a = wc.f_alpha(k)
            pw64, pb64 = wc.accumulated64(G, X, (a, -2.0 * a), ops.dtype)
            what = "%s, rows %d, pair %d of %d (%d x %d, alpha %r)" % (name, rows, k, count, o, i, a)
            _exact_pw(pw, pw64, ops.dtype, what)
            assert (pb is not None) == bias
            if bias:
                _exact_pb(pb, pb64, what)
