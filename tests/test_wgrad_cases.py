"""The operands and references of tests/test_gpu_linear_wgrad.py are what they claim (tests/_wgrad_cases.py), checked on the CPU:

* the reference partial layout: K ranges and tile-column slots sum to the plain G^T X and G.sum(0), empty ranges and slots are zero;
* exact operands: the worst case of every launch sequence stays below 2^24 steps, and every reference value is a number of the state's
  dtype -- so "bit for bit against float64" asks nothing of the order of a sum;
* impulse operands: every element of dW is one product that fp32 holds, the six kept part products add up to it and the three dropped
  ones are zero; the impulses reach every K range, both K halves and the last existing row;
* the power-of-two scalings: no part of the split and none of the six kept products is subnormal or overflows;
* the poisoned positions are where the cases say; the wide group passes the launcher's rule on 256 CUs; the guards hold what they say."""
import pytest
import torch

import _linear_tile_cases as tc
import _wgrad_cases as wc

_WIDE = [(r,) + wc.WIDE_GROUP[0] + (k,) for r in sorted(set(wc.A_WIDE_ROWS + wc.B_WIDE_ROWS)) for k in range(len(wc.WIDE_GROUP))]
_EXACT_SHAPES = sorted(set([c + (0,) for c in wc.A_CASES + wc.B_CASES] + _WIDE))       # (rows, out_f, in_f, pair of its group)


def test_kper_and_the_wide_rule():
    assert [wc.kper(r) for r in (256, 257, 289, 319, 320, 512, 768, 1000, 1024, 4096)] == [32, 64, 64, 64, 64, 64, 96, 128, 128, 512]
    assert [wc.is_ragged(r) for r in (256, 257, 320, 512, 768, 1000)] == [False, True, True, False, False, True]
    assert wc.takes_wide(wc.WIDE_GROUP, 256) and not wc.takes_wide(wc.WIDE_GROUP[:1], 256)            # 256 workgroups; 128 do not fill the chip
    assert not wc.takes_wide([(512, 512), (512, 512), (128, 128)], 256)                               # 264: most of a second round idle
    assert not wc.takes_wide([(512, 512), (512, 576)], 256) and wc.takes_wide([(512, 512)] * 4, 256)
    assert not any(wc.takes_wide([(o, i)], 256) for _, o, i in wc.A_CASES + wc.B_CASES)
    # every row class and every index path the issue lists is there
    rows = set(r for r, _, _ in wc.A_CASES)
    assert rows == {256, 257, 289, 319, 320, 512, 768, 1000} and set(wc.A_WIDE_ROWS) >= {256, 257, 512, 768, 1000}
    assert {(o, i) for _, o, i in wc.A_CASES} == {(64, 64), (128, 64), (64, 192), (128, 512)}
    assert all(wc.is_ragged(r) for r, _, _ in wc.B_CASES[:-1]) and wc.B_CASES[-1] == (256, 128, 64)
    # no sequence of launches cancels: the accumulated alpha is not zero
    assert all(sum(wc.alphas_for(r)) != 0 for r in rows | set(wc.A_WIDE_ROWS))


@pytest.mark.parametrize("rows,out_f,in_f,pair", _EXACT_SHAPES)
def test_exact_cases_are_exact_and_the_layout_sums_to_the_plain_product(rows, out_f, in_f, pair):
    alphas = wc.alphas_for(rows)
    worst, limit = wc.exactness_margin(rows, alphas)
    assert worst < limit, (worst, limit)
    G, X = wc.exact_layers(rows, [(out_f, in_f)] * (pair + 1))[pair]
    assert float(G.abs().max()) <= 62.0 and float(X.abs().max()) <= 62.0 and torch.equal(2 * G, (2 * G).round())
    ntn, kp = in_f // wc.BN, wc.kper(rows)
    plain_w, plain_b = G.double().t() @ X.double(), G.double().sum(0)
    # the layout, once (alpha 1): every K range and every slot against the rows and slabs it stands for
    pw, pb = wc.partials64(G, X, 1.0)
    assert pw.shape == (8, out_f, in_f) and pb.shape == (8, ntn, out_f)
    assert torch.equal(pw.sum(0), plain_w) and torch.equal(pb.sum((0, 1)), plain_b)
    for s in range(8):
        lo, hi = s * kp, min((s + 1) * kp, rows)
        if lo >= rows:                                             # a K range past the rows: exactly zero
            assert not bool(pw[s].any()) and not bool(pb[s].any())
            continue
        assert torch.equal(pw[s], G[lo:hi].double().t() @ X[lo:hi].double())
        for j in range(ntn):
            mine = [t for t in range(kp // wc.SLAB) if t % ntn == j and lo + t * wc.SLAB < rows]
            want = sum((G[lo + t * wc.SLAB:min(lo + (t + 1) * wc.SLAB, rows)].double().sum(0) for t in mine), torch.zeros(out_f, dtype=torch.float64))
            assert torch.equal(pb[s, j], want)
            assert mine or not bool(pb[s, j].any())
    # the alphas are powers of two and G is the same number in either dtype: every launch is alpha times that layout, in both dtypes
    for a in alphas:
        assert torch.equal(wc.scaled(G, a, torch.float32), a * G.double()) and torch.equal(wc.scaled(G, a, torch.float64), a * G.double())
    total = sum(alphas)
    acc_w, acc_b = total * pw, total * pb
    if (rows, out_f, in_f) in wc.A_CASES[:3]:                      # (and accumulated64 is that sum, launch by launch)
        for dtype in (torch.float32, torch.float64):
            w, b = wc.accumulated64(G, X, alphas, dtype)
            assert torch.equal(w, acc_w) and torch.equal(b, acc_b)
    assert wc.is_exact_in(acc_w, torch.float32) and wc.is_exact_in(acc_b, torch.float32)
    # what the kernels are compared with is not zero: every K range that has rows holds non-zero entries -- most of them -- and slots
    for s in range(8):
        if s * kp < rows:
            assert int((acc_w[s] != 0).sum()) > acc_w[s].numel() // 2, s
            assert bool(acc_b[s].any()), s
    mu_w, mu_b = wc.mu_start(out_f, in_f, wc.seed_of(rows, out_f, in_f))
    assert wc.is_exact_in(mu_w.double() + acc_w.sum(0), torch.float32) and wc.is_exact_in(mu_b.double() + acc_b.sum((0, 1)), torch.float32)
    assert bool((acc_w.sum(0) != 0).any()) and bool((acc_b.sum((0, 1)) != 0).any())                # mu moves
    # the sum in fp32, K ranges in order and reversed, as the kernels and any other order would form it
    w32 = acc_w.float()
    up = sum((w32[s] for s in range(8)), torch.zeros(out_f, in_f))
    down = sum((w32[s] for s in range(7, -1, -1)), torch.zeros(out_f, in_f))
    assert torch.equal(up.double(), total * plain_w) and torch.equal(down.double(), total * plain_w)


def test_most_pb_slots_of_the_widest_case_stay_zero():
    G, X = wc.exact_operands(256, 128, 512)
    _, pb = wc.partials64(G, X, 1.0)
    assert bool(pb[:, 0].all()) and not bool(pb[:, 1:].any())      # one slab per range: tile column 0 owns it, seven slots stay zero
    G, X = wc.exact_operands(257, 64, 64)
    pw, pb = wc.partials64(G, X, 1.0)
    assert torch.equal(pw[4], G[256:].double().t() @ X[256:].double()) and not bool(pw[5:].any()) and torch.equal(pb[4, 0], G[256].double())


@pytest.mark.parametrize("count", wc.F_COUNTS)
@pytest.mark.parametrize("rows", wc.F_ROWS)
def test_group_cases_are_exact(rows, count):
    assert len(wc.F_SHAPES) == max(wc.F_COUNTS) == 10 and len(set(wc.F_SHAPES)) == 10
    assert len({wc.f_alpha(k) for k in range(10)}) == 10
    for k, (out_f, in_f, _) in enumerate(wc.F_SHAPES[:count]):
        a = wc.f_alpha(k)
        assert torch.frexp(torch.tensor(abs(a)))[0] == 0.5           # a power of two
        alphas = (a, -2.0 * a)
        worst, limit = wc.exactness_margin(rows, alphas)
        assert worst < limit
        G, X = wc.exact_operands(rows, out_f, in_f, wc.seed_of(rows, out_f, in_f) + k)
        for dtype in (torch.float32, torch.float64):
            pw, pb = wc.accumulated64(G, X, alphas, dtype)
            assert wc.is_exact_in(pw, dtype) and wc.is_exact_in(pb, torch.float32)
            assert torch.equal(pw.sum(0), -a * (G.double().t() @ X.double())) and torch.equal(pb.sum((0, 1)), -a * G.double().sum(0))


# ---- C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", sorted(set(r for _, r, _, _ in wc.C_CASES) | set(r for _, r in wc.C_WIDE_CASES)))
def test_the_impulses_reach_every_range_both_halves_and_the_last_row(rows):
    cand = wc.impulse_rows(rows)
    kp = wc.kper(rows)
    assert cand[0] == rows - 1 and len(set(cand)) == len(cand) and max(cand) < rows
    for s in range(8):
        for t in range(kp // wc.SLAB):
            for h in (0, 1):
                lo = s * kp + t * wc.SLAB + h * wc.HALF
                there = [k for k in cand if lo <= k < lo + wc.HALF]
                assert there or lo + wc.HALF > rows, (s, t, h)     # a half with all its rows has an impulse; a ragged one may have rows - 1 only
    sizes = [o for _, r, o, _ in wc.C_CASES if r == rows] + [i for kind, r, _, i in wc.C_CASES if r == rows and kind == "x-onehot"]
    sizes += [wc.WIDE_GROUP[0][0] for _, r in wc.C_WIDE_CASES if r == rows]
    for n in sizes:
        assert set(wc.impulse_map(rows, n).tolist()) == set(cand), n                  # every impulse row is used


_C_ALL = [c + (0,) for c in wc.C_CASES] + [(kind, r) + wc.WIDE_GROUP[0] + (k,) for kind, r in wc.C_WIDE_CASES for k in range(len(wc.WIDE_GROUP))]


@pytest.mark.parametrize("kind,rows,out_f,in_f,pair", _C_ALL)
def test_every_element_of_an_impulse_case_is_one_exact_product(kind, rows, out_f, in_f, pair):
    G, X, alpha, bias = wc.impulse_operands(kind, rows, out_f, in_f, wc.pair_seed(rows, out_f, in_f, pair))
    a, b = wc.impulse_factors(kind, G, X, alpha)
    assert bool((a != 0).all()) and bool((b != 0).all())
    prod = a.double() * b.double()
    assert wc.is_exact_in(prod, torch.float32) and bool((prod.float() != 0).all()) and bool(torch.isfinite(prod.float()).all())
    # the reference in the partial layout is that product, each element in the K range of its impulse row
    pw, pb = wc.partials64(G, X, alpha)
    assert torch.equal(pw.sum(0), prod) and wc.is_exact_in(pw, torch.float32)
    assert int((pw != 0).sum()) == out_f * in_f                    # one K range per element
    if bias:
        assert wc.is_exact_in(pb, torch.float32) and int((pb != 0).sum()) == out_f
    # the split: the six kept products are the product, the three dropped ones nothing
    assert torch.equal(wc.part_products64(a, b, tc.SIX), prod)
    pa, pb3 = tc.split3(a), tc.split3(b)
    for i, j in wc.DROPPED:
        assert not bool((pa[i].double() * pb3[j].double()).any()), (i, j)
    # ... and each kind needs the terms it is there for: without them the sum is another number everywhere / somewhere
    needs = {"g-onehot": [(0, 1), (0, 2)], "x-onehot": [(1, 0), (2, 0)], "mid-mid": [(1, 1)], "alpha-0.3": [(1, 0), (2, 0)], "subnormal": [(0, 1), (0, 2)]}[kind]
    for term in needs:
        kept = [p for p in tc.SIX if p != term]
        assert bool((wc.part_products64(a, b, kept) != prod).any()), term
    # fp64 states: the same operands, scaled in double
    pw64, _ = wc.partials64(G, X, alpha, torch.float64)
    assert torch.equal(pw64.sum(0), wc.scaled(G, alpha, torch.float64).t() @ X.double())


def test_the_parts_of_the_mid_mid_and_subnormal_operands():
    hi, mid, lo = tc.split3(torch.tensor([1.0 + 2.0 ** -8]))
    assert (float(hi), float(mid), float(lo)) == (1.0, 2.0 ** -8, 0.0)
    hi, mid, lo = tc.split3(torch.tensor([2.0 ** -130]))
    assert (float(hi), float(mid), float(lo)) == (2.0 ** -130, 0.0, 0.0) and float(hi) < 2.0 ** -126
    hi, mid, lo = tc.split3(torch.tensor([2.0 ** 100 * (1.0 + 2.0 ** -8 + 2.0 ** -16)]))
    assert (float(hi), float(mid), float(lo)) == (2.0 ** 100, 2.0 ** 92, 2.0 ** 84)
    a, b = torch.tensor([2.0 ** -130]), torch.tensor([2.0 ** 100 * (1.0 + 2.0 ** -8 + 2.0 ** -16)])
    assert float(wc.part_products64(a, b, tc.SIX)) == 2.0 ** -30 * (1.0 + 2.0 ** -8 + 2.0 ** -16)
    assert float(wc.part_products64(a, b, tc.SIX, flush_subnormal_parts=True)) == 0.0
    assert float(torch.tensor(0.3, dtype=torch.float32) * torch.tensor(4.0)) == float(torch.tensor(0.3, dtype=torch.float32)) * 4.0


# ---- D ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,out_f,in_f", wc.SCALING_CASES + [(r,) + wc.WIDE_GROUP[0] for r in wc.SCALING_WIDE_ROWS])
def test_no_term_of_a_scaled_wgrad_product_is_subnormal_or_overflows(rows, out_f, in_f):
    for k in range(2 if (out_f, in_f) == wc.WIDE_GROUP[0] else 1):
        G, X = wc.normal_operands(rows, out_f, in_f, wc.seed_of(rows, out_f, in_f) + k)
        assert G.shape == (rows, out_f) and X.shape == (rows, in_f)
        assert wc.scaling_is_exact(G, X, 0, 0)
        for p, q in tc.SCALINGS:
            assert wc.scaling_is_exact(G, X, p, q), (p, q)
    assert not wc.scaling_is_exact(G, X, -90, -90) and not wc.scaling_is_exact(G, X, 70, 70)


def test_the_rolls_move_whole_k_ranges():
    for rows, _, _ in wc.ROLL_CASES + [(r, 0, 0) for r in wc.ROLL_WIDE_ROWS]:
        assert not wc.is_ragged(rows) and wc.kper(rows) % wc.SLAB == 0 and rows in (512, 768)
        G, X = wc.normal_operands(rows, 64, 64)
        shift = wc.ROLL_RANGES * wc.kper(rows)
        pw, pb = wc.partials64(G, X, 1.0)
        pwr, pbr = wc.partials64(G.roll(shift, 0), X.roll(shift, 0), 1.0)
        assert torch.equal(pwr, pw.roll(wc.ROLL_RANGES, 0)) and torch.equal(pbr, pb.roll(wc.ROLL_RANGES, 0)) and not torch.equal(pwr, pw)


# ---- E ---------------------------------------------------------------------------------------------------------------------------------
def test_the_poisoned_positions_are_where_the_cases_say():
    cases = wc.E_CASES + [(r,) + wc.WIDE_GROUP[0] + (at,) for r, at in wc.E_WIDE_CASES]
    assert [wc.is_ragged(c[0]) for c in cases] == [False, True, False, True]
    for rows, out_f, in_f, at in cases:
        ntn = in_f // wc.BN
        assert sorted(wc.place_of(rows, k0)[2] for k0, _, _ in at) == [0, 1]                   # both K halves
        for k0, m0, n0 in at:
            s, t, h = wc.place_of(rows, k0)
            assert k0 < rows and m0 < out_f and n0 < in_f and t % ntn == 1
            if wc.is_ragged(rows):                                 # the last slab, partly filled
                assert s * wc.kper(rows) + (t + 1) * wc.SLAB > rows > s * wc.kper(rows) + t * wc.SLAB
            G, X = wc.normal_operands(rows, out_f, in_f)
            assert bool((G[k0] != 0).all()) and bool((X[k0] != 0).all())   # (a non-finite value times zero would be NaN whatever its kind)
            for kind in wc.POISONS:
                mw, mb = wc.poisoned_masks(kind, rows, out_f, in_f, k0, m0, n0)
                Gp, Xp = G.clone(), X.clone()
                if kind == "nan-x":
                    Xp[k0, n0] = float("nan")
                else:
                    Gp[k0, m0] = {"nan-g": float("nan"), "+inf-g": float("inf"), "-inf-g": float("-inf")}[kind]
                pw, pb = wc.partials64(Gp, Xp, 1.0)
                assert torch.equal(~torch.isfinite(pw), mw) and torch.equal(~torch.isfinite(pb), mb)
                assert int(mw.sum()) == (out_f if kind == "nan-x" else in_f) and int(mb.sum()) == (0 if kind == "nan-x" else 1)


# ---- B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_guarded_flat(dtype):
    for n, guard, skew in ((8 * 128 * 64, 128 * 64, 0), (128, 64, 1), (64, 70, 1)):
        words, view, span = wc.guarded_flat(n, guard, dtype, "cpu", skew)
        size = view.element_size()
        assert view.numel() == n and view.dtype == dtype and view.is_contiguous()
        assert (view.data_ptr() - words.data_ptr()) == span[0] * 4 and (span[1] - span[0]) * 4 == n * size
        assert words.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (skew * size) % 16 and (skew == 0 or view.data_ptr() % 16 != 0)
        assert span[0] * 4 >= guard * size and (words.numel() - span[1]) * 4 >= guard * size
        assert wc.guards_ok(words, span) and (dtype == torch.float64 or bool(torch.isnan(view).all()))
        view.zero_()
        assert wc.guards_ok(words, span)
        words[span[0] - 1] = 0
        assert not wc.guards_ok(words, span)
        words[span[0] - 1] = tc.SENTINEL
        words[span[1]] = 0
        assert not wc.guards_ok(words, span)


def test_first_wrong_names_range_tile_and_element():
    want = torch.zeros(8, 128, 192)
    got = want.clone()
    assert wc.first_wrong(got, want) is None
    got[5, 70, 130] = 2.0
    got[6, 0, 0] = 1.0
    assert wc.first_wrong(got, want) == (5, (1, 2), (70, 130), 2.0, 0.0, 2)
