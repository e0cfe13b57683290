"""TEST SCAFFOLDING -- operands, float64 references and premises of the tests of pn_linear_wgrad_group / pn_linear_wgrad_finish
(csrc/pn_linear.hip): tests/test_wgrad_cases.py checks on the CPU that they are what they claim, tests/test_gpu_linear_wgrad.py runs the
kernels on them.  Importable without a GPU; every builder returns CPU tensors.  `distinct`, `normal`, `split3`, `SIX`, `SENTINEL` and
`SCALINGS` are those of tests/_linear_tile_cases.py.

A case is (rows, out_f, in_f): G is rows x out_f (the cotangent), X rows x in_f (the layer's input).  The K dimension -- the rows -- is cut
into eight K ranges of `kper` rows, a range into slabs of 32 rows, a slab into two K halves of 16 rows.  The partial buffers:
pw.view(8, out_f, in_f)[s] holds K range s; pb.view(8, ntn, out_f)[s][j], ntn = in_f / 64, holds the column sums of alpha G over the slabs
t of range s with t % ntn == j (the workgroup of tile column j adds them up)."""
import torch

import _linear_tile_cases as tc

KSPLIT, SLAB, HALF, BM, BN = 8, 32, 16, 64, 64
EXACT_FP32, TILE_64 = 1, 2            # PN_WGRAD_EXACT_FP32, PN_WGRAD_TILE_64

# (name, the state's dtype, wgrad_flags) of the 64 x 64 forms; rows decide between the aligned and the ragged instantiation of each
FORMS = [("split", torch.float32, 0), ("split-tile64", torch.float32, TILE_64), ("exact-fp32", torch.float32, EXACT_FP32),
         ("fp64", torch.float64, 0)]
FP32_FORMS = FORMS[:3]
# the 128 x 128 form is the launcher's own choice: flags 0 and a group that fills whole rounds of the chip.  On 256 CUs the smallest one:
WIDE_GROUP = [(512, 512), (512, 512)]


def is_ragged(rows):
    return rows % (KSPLIT * SLAB) != 0


def kper(rows):
    """Rows of a K range: whole slabs; the rows past `rows` of a ragged launch are read as zeros."""
    return -(-rows // (KSPLIT * SLAB)) * SLAB if is_ragged(rows) else rows // KSPLIT


def takes_wide(shapes, cus):
    """The launcher's rule for the 128 x 128 form (flags 0, fp32): every out_f and in_f a multiple of 128, at least one workgroup per CU,
    at most a sixth of the rounds' places idle."""
    if any(o % 128 or i % 128 for o, i in shapes):
        return False
    wblocks = sum((o // 128) * (i // 128) * KSPLIT for o, i in shapes)
    rounds = -(-wblocks // cus)
    return wblocks >= cus and rounds * cus * 5 <= wblocks * 6


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
# A: rows -- 256 one slab per K range; 257 kper = 64, ranges 5-7 empty, row 256 alone in range 4; 289 / 319 / 320 the last slab partly
# filled or absent; 512 two slabs; 768 three (odd); 1000 ragged, four slabs.  (out_f, in_f) -- (64, 64) one tile; (64, 192) ntn = 3, which
# does not divide the slab count; (128, 512) ntn = 8, more than the slabs of a range: most PB slots stay zero.
A_CASES = [(256, 64, 64), (256, 128, 512), (257, 64, 64), (257, 128, 64), (289, 64, 192), (319, 128, 64), (320, 64, 192), (320, 128, 512),
           (512, 64, 192), (512, 128, 64), (768, 64, 192), (768, 128, 512), (1000, 64, 192), (1000, 128, 512)]
A_WIDE_ROWS = [256, 257, 320, 512, 768, 1000]
# B: the ragged shapes and one aligned one, every buffer inside guards
B_CASES = [(257, 128, 64), (257, 64, 192), (289, 64, 192), (319, 128, 64), (320, 64, 192), (1000, 128, 64), (256, 128, 64)]
B_WIDE_ROWS = [257, 256]
# C: (kind, rows, out_f, in_f); out_f is at least the number of impulse rows, so every one of them is used
C_KINDS = ["g-onehot", "x-onehot", "mid-mid"]
C_CASES = [(kind, r, o, i) for r, o, i in [(256, 64, 64), (289, 64, 192), (768, 128, 64), (1000, 128, 64)] for kind in C_KINDS] + \
          [("alpha-0.3", 289, 64, 192), ("alpha-0.3", 512, 128, 64), ("subnormal", 289, 64, 192)]
C_WIDE_CASES = [(kind, r) for r in (256, 289) for kind in C_KINDS] + [("alpha-0.3", 289), ("subnormal", 289)]
# D
SCALING_CASES = [(256, 128, 64), (257, 64, 192)]
SCALING_WIDE_ROWS = [256, 257]
ROLL_CASES = [(512, 64, 192), (768, 128, 64)]
ROLL_WIDE_ROWS = [512, 768]
ROLL_RANGES = 3
# E: (rows, out_f, in_f, [(k0, m0, n0)]): k0 in slab 1 of a K range (so that the tile column owning it is not column 0), once in each K
# half; 512 rows aligned, 319 rows the last, partly filled slab (rows 288 .. 318 of range 4)
E_CASES = [(512, 128, 192, [(229, 70, 130), (245, 5, 63)]), (319, 128, 192, [(290, 70, 130), (310, 127, 64)])]
E_WIDE_CASES = [(512, [(229, 200, 333), (245, 70, 130)]), (319, [(290, 200, 333), (310, 511, 64)])]
POISONS = ["nan-g", "nan-x", "+inf-g", "-inf-g"]
# F: (out_f, in_f, bias) of up to ten pairs, two launches beyond eight
F_SHAPES = [(64, 192, False), (128, 64, True), (64, 64, False), (192, 128, True), (64, 128, True), (128, 128, True), (256, 64, True),
            (64, 256, False), (128, 192, True), (192, 64, True)]
F_COUNTS = [1, 4, 8, 10]
F_ROWS = [256, 289]


def f_alpha(k):
    """A different power of two per pair, 1/8 .. 2 (from 4 on the half steps of mu would be the finer ones)."""
    return 2.0 ** ((k * 3) % 5 - 3) * (-1.0 if k % 2 else 1.0)


def seed_of(rows, out_f, in_f):
    return rows + 3 * out_f + 7 * in_f


# ---- exact operands: the premise ---------------------------------------------------------------------------------------------------
def alphas_for(rows):
    """The accumulating launches of an exact case: 1 then -2 while the worst case stays exact; up to 512 rows 1 twice (never a pair that
    cancels: the sum would be zero everywhere, and any error linear in alpha with it); beyond, one launch."""
    return (1.0, -2.0) if rows <= 320 else ((1.0, 1.0) if rows <= 512 else (-2.0,))


def exactness_margin(rows, alphas):
    """(worst case, limit): sum |alpha| rows 62^2 plus a `distinct` mu against 2^24 steps, a step being the smallest |alpha| quarters
    (products of `distinct` values are whole quarters; mu holds whole halves).  Below the limit every partial sum, in any order, and the
    finished mu are fp32 numbers."""
    worst = sum(abs(a) for a in alphas) * rows * 62.0 ** 2 + 62.0
    step = min(0.25 * min(abs(a) for a in alphas), 0.5)
    return worst, 2.0 ** 24 * step


def is_exact_in(t64, dtype):
    return torch.equal(t64.to(dtype).double(), t64)


# ---- the float64 reference, in the layout of the partial buffers ---------------------------------------------------------------------
def scaled(G, alpha, dtype):
    """alpha G as the kernels form it -- one product in the state's precision, before anything else -- as float64."""
    return (G.to(dtype) * torch.tensor(alpha, dtype=dtype)).double()


def partials64(G, X, alpha, dtype=torch.float32):
    """(pw64 (8, out_f, in_f), pb64 (8, ntn, out_f)) of one launch."""
    rows, out_f = G.shape
    in_f = X.shape[1]
    kp, ntn = kper(rows), in_f // BN
    Gp, Xp = torch.zeros(KSPLIT * kp, out_f, dtype=torch.float64), torch.zeros(KSPLIT * kp, in_f, dtype=torch.float64)
    Gp[:rows], Xp[:rows] = scaled(G, alpha, dtype), X.double()
    pw = torch.einsum("skm,skn->smn", Gp.view(KSPLIT, kp, out_f), Xp.view(KSPLIT, kp, in_f))
    slabs = Gp.view(KSPLIT, kp // SLAB, SLAB, out_f).sum(2)
    pb = torch.zeros(KSPLIT, ntn, out_f, dtype=torch.float64)
    for t in range(kp // SLAB):
        pb[:, t % ntn] += slabs[:, t]
    return pw, pb


def accumulated64(G, X, alphas, dtype=torch.float32):
    pw, pb = partials64(G, X, alphas[0], dtype)
    for a in alphas[1:]:
        w, b = partials64(G, X, a, dtype)
        pw, pb = pw + w, pb + b
    return pw, pb


def exact_operands(rows, out_f, in_f, seed=None):
    seed = seed_of(rows, out_f, in_f) if seed is None else seed
    return tc.distinct(rows, out_f, seed), tc.distinct(rows, in_f, seed + 17)


def pair_seed(rows, out_f, in_f, k):
    """The seed of pair k of a group of exact or impulse operands."""
    return seed_of(rows, out_f, in_f) + 13 * k


def exact_layers(rows, shapes):
    """[(G, X)], `distinct`, a seed per pair of the group."""
    return [exact_operands(rows, o, i, pair_seed(rows, o, i, k)) for k, (o, i) in enumerate(shapes)]


def mu_start(out_f, in_f, seed):
    return tc.distinct(out_f, in_f, seed + 29), tc.distinct(1, out_f, seed + 31).view(-1)


def first_wrong(got, want):
    """(K range, tile (m // 64, n // 64), (m, n), got, want, how many) of the first element of an (8, out_f, in_f) partial that differs."""
    bad = (got != want).nonzero()
    if bad.numel() == 0:
        return None
    s, m, n = (int(v) for v in bad[0])
    return s, (m // BM, n // BN), (m, n), float(got[s, m, n]), float(want[s, m, n]), int(bad.shape[0])


# ---- C: one product per element ------------------------------------------------------------------------------------------------------
def impulse_rows(rows):
    """The rows that carry impulses: the last existing row first, then one row of every K half of every slab of every K range, at a place
    within the half that changes from one to the next; those that do not exist are left out."""
    kp, out = kper(rows), [rows - 1]
    for s in range(KSPLIT):
        for t in range(kp // SLAB):
            for h in (0, 1):
                k = s * kp + t * SLAB + h * HALF + (3 * s + 5 * t + 7 * h) % HALF
                if k < rows and k not in out:
                    out.append(k)
    return out


def impulse_map(rows, n):
    """pi(m), m = 0 .. n - 1: the impulse rows in turn."""
    cand = impulse_rows(rows)
    return torch.tensor([cand[m % len(cand)] for m in range(n)])


def _pow2(rows, cols):
    k, n = torch.arange(rows).view(-1, 1), torch.arange(cols).view(1, -1)
    return 2.0 ** ((n + 3 * k) % 9 - 4).float()


def impulse_operands(kind, rows, out_f, in_f, seed=None):
    """(G, X, alpha, bias).  Every element of dW is ONE product g x that fp32 holds exactly:
    g-onehot   G[pi(m)][m] = 2^e, X seeded normal (24-bit significands): needs hi.hi, hi.mid, hi.lo
    x-onehot   the mirror image: needs hi.hi, mid.hi, lo.hi (no bias: the column sums of a normal G are not exact)
    mid-mid    G[pi(m)][m] = 1 + 2^-8 (hi 1, mid 2^-8, lo 0), X = (1 + 2^-8) 2^e everywhere: (1 + 2^-7 + 2^-16) 2^e needs mid.mid
    alpha-0.3  G one-hot powers of two, alpha = 0.3 (the scaled G has 24 bits), X powers of two
    subnormal  g = 2^-130 (a subnormal bf16 as its own hi part), x = 2^100 (1 + 2^-8 + 2^-16): 2^-30 (...)"""
    seed = seed_of(rows, out_f, in_f) if seed is None else seed
    G, X = torch.zeros(rows, out_f), torch.zeros(rows, in_f)
    m, n = torch.arange(out_f), torch.arange(in_f)
    e_m, e_n = 2.0 ** ((m % 7) - 3).float(), 2.0 ** ((n % 7) - 3).float()
    if kind == "g-onehot":
        G[impulse_map(rows, out_f), m] = e_m
        return G, tc.normal(rows, in_f, seed), 1.0, True
    if kind == "x-onehot":
        X[impulse_map(rows, in_f), n] = e_n
        return tc.normal(rows, out_f, seed), X, 1.0, False
    if kind == "mid-mid":
        G[impulse_map(rows, out_f), m] = 1.0 + 2.0 ** -8
        return G, (1.0 + 2.0 ** -8) * _pow2(rows, in_f), 1.0, True
    if kind == "alpha-0.3":
        G[impulse_map(rows, out_f), m] = e_m
        return G, _pow2(rows, in_f), 0.3, True
    assert kind == "subnormal", kind
    G[impulse_map(rows, out_f), m] = 2.0 ** -130
    return G, torch.full((rows, in_f), 2.0 ** 100 * (1.0 + 2.0 ** -8 + 2.0 ** -16)), 1.0, True


def impulse_factors(kind, G, X, alpha):
    """(a, b), both out_f x in_f fp32: the two factors of every element of dW, a from alpha G (scaled in fp32), b from X."""
    Ga = G * torch.tensor(alpha, dtype=torch.float32)
    out_f, in_f = G.shape[1], X.shape[1]
    if kind == "x-onehot":
        pi = impulse_map(G.shape[0], in_f)
        return Ga[pi].t().contiguous(), X[pi, torch.arange(in_f)].view(1, -1).expand(out_f, in_f).contiguous()
    pi = impulse_map(G.shape[0], out_f)
    return Ga[pi, torch.arange(out_f)].view(-1, 1).expand(out_f, in_f).contiguous(), X[pi].contiguous()


DROPPED = [(1, 2), (2, 1), (2, 2)]     # the three of the nine part products that six_products leaves out


def part_products64(a, b, pairs, flush_subnormal_parts=False):
    """sum over `pairs` of part i of a times part j of b, in float64 (every such product is exact there); with the flag, parts that are
    subnormal bf16 numbers count as zero."""
    pa, pb = tc.split3(a), tc.split3(b)
    if flush_subnormal_parts:
        pa, pb = ([torch.where(p.abs() < 2.0 ** -126, torch.zeros_like(p), p) for p in ps] for ps in (pa, pb))
    total = torch.zeros(a.shape, dtype=torch.float64)
    for i, j in pairs:
        total = total + pa[i].double() * pb[j].double()
    return total


# ---- D: the premise of the power-of-two scalings -----------------------------------------------------------------------------------
def normal_operands(rows, out_f, in_f, seed=None):
    seed = seed_of(rows, out_f, in_f) if seed is None else seed
    return tc.normal(rows, out_f, seed + 1), tc.normal(rows, in_f, seed + 2)


def scaling_is_exact(G, X, p, q):
    """Scaled by 2^p and 2^q: every part of the split of either operand is a normal number or zero, the smallest of the six kept products
    is normal (a lower bound, over all pairs of parts), and rows times the largest product is finite."""
    tiny, huge = 2.0 ** -126, 2.0 ** 127
    Gs, Xs = G * 2.0 ** p, X * 2.0 ** q
    if not (torch.equal(Gs.double(), G.double() * 2.0 ** p) and torch.equal(Xs.double(), X.double() * 2.0 ** q)):
        return False
    pg, px = tc.split3(Gs), tc.split3(Xs)

    def smallest(t):
        return float(t.abs()[t != 0].double().min())
    if not (torch.equal(pg[0] + pg[1] + pg[2], Gs) and torch.equal(px[0] + px[1] + px[2], Xs)):
        return False
    if min(smallest(t) for t in pg + px) < tiny or min(smallest(pg[i]) * smallest(px[j]) for i, j in tc.SIX) < tiny:
        return False
    return G.shape[0] * float(pg[0].abs().double().max()) * float(px[0].abs().double().max()) < huge


# ---- E: where a poisoned operand may show ---------------------------------------------------------------------------------------------
def place_of(rows, k0):
    """(K range, slab within the range, K half) of row k0."""
    kp = kper(rows)
    return k0 // kp, (k0 % kp) // SLAB, (k0 % SLAB) // HALF


def poisoned_masks(kind, rows, out_f, in_f, k0, m0, n0):
    """(mask of pw (8, out_f, in_f), mask of pb (8, ntn, out_f)): the elements a non-finite G[k0][m0] or X[k0][n0] reaches."""
    s, t, _ = place_of(rows, k0)
    ntn = in_f // BN
    mw, mb = torch.zeros(KSPLIT, out_f, in_f, dtype=torch.bool), torch.zeros(KSPLIT, ntn, out_f, dtype=torch.bool)
    if kind == "nan-x":
        mw[s, :, n0] = True
    else:
        mw[s, m0, :] = True
        mb[s, t % ntn, m0] = True
    return mw, mb


# ---- B: guarded buffers ---------------------------------------------------------------------------------------------------------------
def guarded_flat(n, guard, dtype, device, skew=0):
    """(words, view, (first, last)): `view` is n elements of `dtype` inside the int32 buffer `words`, at least `guard` elements of it on
    either side, every word pre-filled with SENTINEL; the view starts on a 16-byte boundary plus `skew` elements and covers
    words[first:last]."""
    ws = 1 if dtype == torch.float32 else 2
    lead = -(-guard // 4) * 4 + skew
    words = torch.full(((lead + n + guard + 4) * ws,), tc.SENTINEL, dtype=torch.int32, device=device)
    first, last = lead * ws, (lead + n) * ws
    return words, words[first:last].view(dtype), (first, last)


def guards_ok(words, span):
    return bool((words[:span[0]] == tc.SENTINEL).all()) and bool((words[span[1]:] == tc.SENTINEL).all())
