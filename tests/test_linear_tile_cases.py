"""The operands of tests/test_gpu_linear_tiles.py are what they claim (tests/_linear_tile_cases.py), checked on the CPU:

* exact operands: the fp32 product, summed over k in natural order, in reversed order and in a fixed permutation, equals the float64 product
  cast to fp32 -- "exact in any order" as a fact, for every (kind, rows, width, K) that the GPU tests compare with float64;
* `distinct`: no two positions of a tile's row (32 k) or column (64 rows) hold the same value;
* the backward's exact case: gz itself is an fp32 number;
* the power-of-two scalings: no term of the kernels' split and none of the six products they keep is subnormal or overflows;
* the shapes reach what they are listed for: the workgroup counts, and a rotation that is a bijection and not the identity."""
import pytest
import torch

import _linear_tile_cases as tc


def _orders(k):
    return {"natural": list(range(k)), "reversed": list(range(k - 1, -1, -1)),
            "permuted": torch.randperm(k, generator=torch.Generator().manual_seed(k)).tolist()}


def _fp32_product(a, bt, order, start=None):
    """sum_k a[:, k] bt[k, :] in fp32, one rounded product and one rounded sum per k, in the given order of k."""
    acc = torch.zeros(a.shape[0], bt.shape[1]) if start is None else start.clone()
    for k in order:
        acc = acc + a[:, k:k + 1] * bt[k:k + 1, :]
    return acc


_SHAPES = sorted(set((r, w, k) for _, r, w, k in tc.exact_cases()))


@pytest.mark.parametrize("rows,width,k", _SHAPES)
def test_forward_products_of_distinct_operands_are_exact_in_any_order(rows, width, k):
    x, w, b = tc.forward_operands("distinct", rows, width, k, tc.case_seed(rows, width, k))
    assert x.dtype == w.dtype == b.dtype == torch.float32 and x.shape == (rows, k) and w.shape == (width, k) and b.shape == (width,)
    z64, zb64 = tc.forward64(x, w), tc.forward64(x, w, b)
    assert torch.equal(z64.float().double(), z64) and torch.equal(zb64.float().double(), zb64)
    wt = w.t().contiguous()
    for name, order in _orders(k).items():
        z = _fp32_product(x, wt, order)
        assert torch.equal(z, z64.float()), name
        assert torch.equal(z + b, zb64.float()), name                                         # the bias last, as the kernel adds it
        assert torch.equal(_fp32_product(x, wt, order, b.expand(rows, width)), zb64.float()), name   # and first


@pytest.mark.parametrize("rows,width,k", _SHAPES)
def test_the_backwards_exact_case_is_exact_in_any_order(rows, width, k):
    g, a, w = tc.backward_operands("distinct", rows, width, k, tc.case_seed(rows, width, k))
    assert g.shape == a.shape == (rows, k) and w.shape == (k, width) and w.is_contiguous()
    assert set(a.unique().tolist()) == {0.0, 1.0}
    z64, dx64 = tc.backward64(g, a, w)
    assert torch.equal(z64.float().double(), z64)                  # gz64.float() == gz64 exactly
    assert torch.equal(z64.float(), g * (1.0 - a * a))             # and the fp32 expression gives it, with or without an fma
    assert bool((z64 == 0).any()) and bool((z64 != 0).any())
    assert torch.equal(dx64.float().double(), dx64)
    z = z64.float()
    for name, order in _orders(k).items():
        assert torch.equal(_fp32_product(z, w, order), dx64.float()), name


@pytest.mark.parametrize("seed", [0, 5, 17, 22, 1000 + 3 * 192 + 7 * 128])
def test_distinct_repeats_no_value_within_a_tiles_row_or_column(seed):
    v = tc.distinct(1024, 320, seed)
    assert bool((v != 0).all()) and float(v.abs().max()) <= 62.0 and torch.equal(v * 2, (v * 2).round())
    # five significant bits: v = m 2^e with m < 32
    m, _ = torch.frexp(v.abs())
    assert torch.equal(m * 32, (m * 32).round())
    for k0 in range(0, 320, tc.SLAB):                              # every row of every K slab
        s = v[:, k0:k0 + tc.SLAB].sort(dim=1).values
        assert not bool((s[:, 1:] == s[:, :-1]).any())
    for r0 in range(0, 1024, tc.TILE_M):                           # every column of every tile row
        s = v[r0:r0 + tc.TILE_M].sort(dim=0).values
        assert not bool((s[1:] == s[:-1]).any())
    # signs alternate along both directions
    assert bool((v[:, 1:] * v[:, :-1] < 0).all()) and bool((v[1:] * v[:-1] < 0).all())


def test_normal_operands_are_seeded_and_scaled():
    x, w, b = tc.forward_operands("normal", 257, 192, 64, 3)
    x2, w2, b2 = tc.forward_operands("normal", 257, 192, 64, 3)
    assert torch.equal(x, x2) and torch.equal(w, w2) and torch.equal(b, b2)
    assert abs(float(x.std()) - 1.0) < 0.05 and abs(float(w.std()) * 8.0 - 1.0) < 0.05
    g, a, wb = tc.backward_operands("normal", 257, 192, 64, 3)
    assert wb.shape == (64, 192) and float(a.abs().max()) < 1.0 and abs(float(wb.std()) * 8.0 - 1.0) < 0.05


@pytest.mark.parametrize("rows,width,k", tc.SCALING_CASES)
def test_no_term_of_a_scaled_product_is_subnormal_or_overflows(rows, width, k):
    """Every part of the split of 2^p A and 2^q B is a normal number or zero, the smallest of the six kept products is at least the
    product of the smallest parts (a lower bound, taken over all pairs) and normal, and K times the largest product is finite."""
    tiny, huge = 2.0 ** -126, 2.0 ** 127
    seed = tc.case_seed(rows, width, k)
    x, w, _ = tc.forward_operands("normal", rows, width, k, seed)
    g, a, wb = tc.backward_operands("normal", rows, width, k, seed)
    for A, B in ((x, w), (tc.gz64(g, a).float(), wb)):
        for p, q in tc.SCALINGS:
            As, Bs = A * 2.0 ** p, B * 2.0 ** q
            assert torch.equal(As.double(), A.double() * 2.0 ** p) and torch.equal(Bs.double(), B.double() * 2.0 ** q)
            pa, pb = tc.split3(As), tc.split3(Bs)
            assert torch.equal(pa[0] + pa[1] + pa[2], As) and torch.equal(pb[0] + pb[1] + pb[2], Bs)

            def smallest(t):
                return float(t.abs()[t != 0].double().min())
            for t in pa + pb:
                assert smallest(t) >= tiny
            assert min(smallest(pa[i]) * smallest(pb[j]) for i, j in tc.SIX) >= tiny, (p, q)
            assert k * float(pa[0].abs().double().max()) * float(pb[0].abs().double().max()) < huge, (p, q)


def test_split3_matches_three_truncations():
    v = torch.tensor([1.0, -3.1415927, 1e-20, 6.5e10, 0.0])
    hi, mid, lo = tc.split3(v)
    assert torch.equal(hi + mid + lo, v)
    for t in (hi, mid, lo):
        assert bool(((t.view(torch.int32) & 0xFFFF) == 0).all())        # each is a bf16
    assert torch.equal(hi, torch.tensor([1.0, -3.140625, float(hi[2]), float(hi[3]), 0.0]))


def test_the_tile_cases_reach_what_they_are_listed_for():
    wg = [tc.workgroups(r, w) for r, w, _ in tc.TILE_CASES]
    assert wg == [16, 16, 48, 16, 16, 32, 9]
    assert [tc.is_aligned(r, w) for r, w, _ in tc.TILE_CASES] == [True, True, True, False, False, False, True]
    for n in wg:
        tiles = [tc.rotated_tile(b, n) for b in range(n)]
        assert sorted(tiles) == list(range(n))                     # a bijection
        assert (tiles != list(range(n))) == (n % 8 == 0)           # and, on a multiple of 8 above 8, not the identity
    assert [tc.rotated_tile(b, 8) for b in range(8)] == list(range(8))     # what every earlier kernel test ran
    # the workgroups that share a 64-row slab of x land on one XCD (bid % 8) when the tile columns divide nblk / 8
    for rows, width, _ in tc.TILE_CASES[:3]:
        n, ntn = tc.workgroups(rows, width), width // tc.TILE_N
        if (n >> 3) % ntn == 0:
            by_row = {}
            for b in range(n):
                by_row.setdefault(tc.rotated_tile(b, n) // ntn, set()).add(b & 7)
            assert all(len(x) == 1 for x in by_row.values())
    # B's row counts: none a multiple of 32, all at least 256; C's include aligned and ragged ones
    assert all(r % 32 and r >= 256 for r in tc.RAGGED_ROWS)
    assert any(tc.is_aligned(r, 128) for r in tc.ROW_COUNTS) and any(not tc.is_aligned(r, 128) for r in tc.ROW_COUNTS)
    assert max(tc.ROW_COUNTS) == tc.MASTER_ROWS
    assert max(max(r, w) for r, w, _ in tc.TILE_CASES) <= 1024 and max(w for _, w, _ in tc.TILE_CASES) <= 512


def test_guarded_and_first_wrong_tile():
    buf, view = tc.guarded(257, 192, "cpu")
    assert view.shape == (257, 192) and view.is_contiguous() and view.data_ptr() % 16 == 0
    assert buf.shape[0] == 257 + tc.GUARD_BEFORE + tc.GUARD_AFTER and tc.GUARD_BEFORE >= 64 and tc.GUARD_AFTER >= 128
    # a whole tile stored one tile row past the last one, its columns running 64 past the ragged width, stays inside
    last_row = -(-257 // tc.TILE_M) * tc.TILE_M + tc.TILE_M - 1
    assert (tc.GUARD_BEFORE + last_row) * 192 + 2 * tc.TILE_N <= buf.numel()
    assert bool(torch.isnan(buf).all()) and tc.guards_untouched(buf, 257)
    view.zero_()
    assert tc.guards_untouched(buf, 257)
    buf[tc.GUARD_BEFORE + 257, 0] = 0.0                            # the row just past the view
    assert not tc.guards_untouched(buf, 257)
    buf, view = tc.guarded(257, 192, "cpu")
    buf[tc.GUARD_BEFORE - 1, 191] = 1.0
    assert not tc.guards_untouched(buf, 257)
    want = torch.zeros(130, 300)
    got = want.clone()
    assert tc.first_wrong_tile(got, want) is None
    got[129, 260] = 1.0
    got[70, 5] = 2.0
    assert tc.first_wrong_tile(got, want) == ((1, 0), (70, 5), 2.0, 0.0, 2)
