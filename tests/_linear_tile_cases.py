"""TEST SCAFFOLDING -- operands and shapes of the tile-map tests of pn_linear_fwd / pn_linear_bwd (csrc/pn_linear.hip):
tests/test_linear_tile_cases.py checks on the CPU that the operands are what they claim, tests/test_gpu_linear_tiles.py runs the kernels on
them, tests/test_gpu_linear_forms.py takes `distinct` from here.  Importable without a GPU; every builder returns CPU tensors.

A case is (rows, width, K): `width` the output's columns (out_f forward, in_f backward), K the product's depth (in_f forward, out_f
backward).  Forward operands: x (rows, K), w (width, K), b (width,).  Backward operands: g, a (rows, K), w (K, width) -- w as it lies,
out_f x in_f.  A workgroup owns 64 rows x 128 columns of the output; a K slab is 32 k."""
import torch

TILE_M, TILE_N, SLAB = 64, 128, 32

# ---- the shapes ------------------------------------------------------------------------------------------------------------------
# A: every tile lands where it belongs.  With a multiple of 8 workgroups the tile index is rotated, (bid & 7) * (nblk >> 3) + (bid >> 3).
TILE_CASES = [
    (512, 256, 64),      # 8 x 2 = 16 workgroups: the smallest rotation that is not the identity; pipelined and (PLAIN) plain
    (1024, 128, 64),     # 16 x 1: one tile column under rotation
    (768, 512, 96),      # 12 x 4 = 48: nblk >> 3 = 6, four tile columns, 3 slabs (an odd number: the plain loop)
    (449, 256, 64),      # 8 x 2: ragged rows under rotation, the last tile row holds one row
    (512, 192, 64),      # 8 x 2: ragged columns under rotation
    (1000, 192, 128),    # 16 x 2 = 32: both ragged, under rotation
    (576, 128, 64),      # 9: no rotation, for contrast
]
# the same 12 x 4 grid at 2 and 4 slabs, which the pipelined loop takes (it needs an even number of them)
EXTRA_TILE_CASES = [(768, 512, 64), (768, 512, 128)]
# B: row counts that are no multiple of 32 (the C/D register map of the 32 x 32 MFMAs and the three row guards), behind guard rows
RAGGED_ROWS = [257, 319, 321, 383]
RAGGED_WIDTH_K = [(128, 64), (192, 64)]
ALIGNED_GUARD_CASE = (256, 128, 64)
# C: one row, many launches
MASTER_ROWS = 513
ROW_COUNTS = [256, 257, 319, 320, 383, 384, 512, 513]
LAUNCH_WIDTH_K = [(128, 128), (192, 64)]
EXTRA_LAUNCH_WIDTH_K = [(128, 96)]    # three slabs: aligned row counts take the plain loop, the others the ragged body
ROLL_ROW_COUNTS = [384, 320]
ROW_ROLL, COL_ROLL = 37, 45
SCALINGS = [(40, 0), (0, -40), (30, -30), (-30, -30), (20, 20)]
SCALING_CASES = [(256, 128, 64), (257, 128, 64)]


def is_aligned(rows, width):
    """The launch takes the pipelined body (or, with PN_LINEAR_FORM_PLAIN or an odd number of K slabs, the plain one); otherwise the
    ragged one, whatever the flag."""
    return rows % TILE_M == 0 and width % TILE_N == 0


def pipelines(k):
    """The pipelined loop takes an even number of slabs."""
    return (k // SLAB) % 2 == 0


def workgroups(rows, width):
    return -(-rows // TILE_M) * -(-width // TILE_N)


def rotated_tile(bid, nblk):
    """The tile a workgroup takes, as both kernel bodies compute it."""
    return (bid & 7) * (nblk >> 3) + (bid >> 3) if nblk % 8 == 0 else bid


# ---- operands --------------------------------------------------------------------------------------------------------------------
def _magnitudes():
    """Every m * 2^e, m = 1 .. 31, e = -1 .. 1, once: 63 values between 1/2 and 62, each of at most five significant bits."""
    return sorted({m * 2.0 ** e for m in range(1, 32) for e in (-1, 0, 1)})


_MAG = torch.tensor(_magnitudes(), dtype=torch.float32)
_NVAL = 2 * _MAG.numel()              # 126 = 2 * 3^2 * 7: 11 and 5 are coprime to it


def distinct(rows, cols, seed):
    """A five-bit value times 2^(-1 .. 1) in every position, signs alternating along rows and columns: entry number (11 r + 5 c + seed) % 126
    of the table +-m 2^e -- any 126 consecutive positions of a row, and of a column, hold 126 different values, so no two positions of a
    tile's row (32 k) or column (64 rows) agree.  |v| <= 62 in steps of 1/2: a product has ten bits below 2^12, a sum of 320 products is
    below 2^21 in steps of 1/4 -- exact in fp32 in any order, a bias of the same kind included."""
    r = torch.arange(rows).view(-1, 1)
    c = torch.arange(cols).view(1, -1)
    i = (11 * r + 5 * c + seed) % _NVAL
    return _MAG[i // 2] * (1 - 2 * (i % 2)).float()


def normal(rows, cols, seed, scale=1.0):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed)) * scale


def forward_operands(kind, rows, width, k, seed):
    """x (rows, k), w (width, k), b (width,): `distinct`, or seeded normal with w scaled by k^-1/2."""
    if kind == "normal":
        return normal(rows, k, seed), normal(width, k, seed + 17, k ** -0.5), normal(1, width, seed + 5).view(-1)
    return distinct(rows, k, seed), distinct(width, k, seed + 17), distinct(1, width, seed + 5).view(-1)


def backward_operands(kind, rows, width, k, seed):
    """g, a (rows, k), w (k, width).  distinct -- the exact case: a in {0, 1}, so 1 - a^2 in {1, 0} and gz is g with every third
    position struck out; normal: a = tanh of a normal draw, w scaled by k^-1/2."""
    if kind == "normal":
        return normal(rows, k, seed), torch.tanh(normal(rows, k, seed + 3)), normal(k, width, seed + 17, k ** -0.5)
    a = ((torch.arange(rows).view(-1, 1) + torch.arange(k).view(1, -1)) % 3 == 0).float()
    return distinct(rows, k, seed), a, distinct(width, k, seed + 17).t().contiguous()


def gz64(g, a):
    return g.double() * (1.0 - a.double() * a.double())


def forward64(x, w, b=None):
    z = x.double() @ w.double().t()
    return z if b is None else z + b.double()


def backward64(g, a, w):
    z = gz64(g, a)
    return z, z @ w.double()


def exact_cases():
    """(kind, rows, width, K) of every launch that is compared with float64 exactly: groups A and B."""
    shapes = TILE_CASES + EXTRA_TILE_CASES + [(r, wd, k) for r in RAGGED_ROWS for wd, k in RAGGED_WIDTH_K] + [ALIGNED_GUARD_CASE]
    return [(kind, r, wd, k) for kind in ("forward", "backward") for r, wd, k in shapes]


def case_seed(rows, width, k):
    return rows + 3 * width + 7 * k


# ---- the split of the kernels, for the premise of the power-of-two scaling test ----------------------------------------------------
def split3(v):
    """The three bf16 terms of an fp32 tensor as split3 of csrc/pn_linear.hip forms them (truncations; hi + mid + lo == v exactly)."""
    def top(t):
        return (t.view(torch.int32) & -65536).view(torch.float32)
    hi = top(v)
    r1 = v - hi
    mid = top(r1)
    lo = top(r1 - mid)
    return hi, mid, lo


# the six products the kernels keep, as (part of the first operand, part of the second): six_products of csrc/pn_linear.hip
SIX = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]


# ---- guarded outputs -------------------------------------------------------------------------------------------------------------
GUARD_BEFORE, GUARD_AFTER = 64, 192
SENTINEL = 0x7FA5C3E1                 # a NaN pattern no result carries


def guarded(rows, cols, device):
    """(buffer, view): `view` is rows x cols, contiguous and 16-byte aligned, with 64 guard rows before it and 192 after it in `buffer`
    (a stray store of a whole 64 x 128 tile one tile row further, its ragged columns running on into the next row, is still inside), every
    word of the buffer pre-filled with SENTINEL."""
    buf = torch.full((GUARD_BEFORE + rows + GUARD_AFTER, cols), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
    return buf, buf[GUARD_BEFORE:GUARD_BEFORE + rows]


def guards_untouched(buf, rows):
    """Both guards of a `guarded` buffer still hold SENTINEL in every word."""
    words = buf.view(torch.int32)
    return bool((words[:GUARD_BEFORE] == SENTINEL).all()) and bool((words[GUARD_BEFORE + rows:] == SENTINEL).all())


def first_wrong_tile(got, want):
    """(row // 64, col // 128) of the first element that differs, with the element's place and both values; None if equal."""
    bad = (got != want).nonzero()
    if bad.numel() == 0:
        return None
    r, c = int(bad[0, 0]), int(bad[0, 1])
    return (r // TILE_M, c // TILE_N), (r, c), float(got[r, c]), float(want[r, c]), int(bad.shape[0])
