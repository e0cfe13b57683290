"""-m gpu: the weighted RMS error norm (pn_combine_wrms_kernel, pn_rows_combine_wrms_kernel, wrms_term<T> in csrc/pn_device.h) and
the row-group widths of the pn_rows_* kernels, where random operands cannot tell a right kernel from a wrong one.

1. Regimes.  tests/_wrms_cases.py builds (un, err) pairs in which the branches of the formula differ -- err below, at and just above
   one ulp of un (the norm is taken between the two STORED solutions), |uhat| above and below |u| and across zero, zero operands,
   atol alone / rtol alone / both, quotients whose square overflows fp32 -- each class also on its own, so small terms are not
   drowned by large ones.  A case is fed as u = un, K_1 = err, ce = [1] (rows: h = 1), first same as last: the kernel's err is K_1
   bit for bit.  A second parametrisation goes through the write path (nk = 3, dyadic operands, every fma exact): unew must be
   the reference's bits.  The reference is wrms_ref (fp64, exactly rounded sum), established on the CPU in
   tests/test_error_norm_host.py.
2. Impulse probes.  One element (or all but one) carries an error: a lost or double-counted element, lane, LDS word or workgroup
   partial changes the norm by a factor, not by 1e-4.  Positions are the seams of the launch geometry.  pn_combine_wrms and pn_dots
   launch one tile per workgroup (no grid cap); the capped grid whose seams are probed is that of csrc/pn_tgrad.hip, and the same
   positions are workgroup seams of the uncapped kernels.
3. Row-group widths.  geom() of csrc/pn_rows.hip gives a row G = 1, 2, ..., 256 threads; every G is run (vector and ragged form),
   with an impulse in every column, and once past the capped grid with a partly live last workgroup.

Tolerances are derived, not measured.  fp32 states: wrms_term<float> rounds atol and rtol to float (on separate addends of tol:
together at most 2^-24 of it), tol takes two further roundings and the quotient is within 2.5 ulp: each q, and so the norm, is
within ~4 * 2^-23 = 5e-7 relative -> 1e-6.  fp64: a few ulp per term and a tree sum of at most 2^22 terms -> 1e-12; a single
non-zero term -> 1e-14.  Exactly zero terms give exactly 0.

Not covered on purpose: fp32 denormal operands; atol below fp32 range; tol == 0 (the reference itself divides by zero)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _wrms_cases as wc
from conftest import require_gpu
from pnode_amd import _lib
from pnode_amd._vecops import HipVecOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
NP = {torch.float32: np.float32, torch.float64: np.float64}
REL = {torch.float32: 1e-6, torch.float64: 1e-12}
REL_ONE = {torch.float32: 1e-6, torch.float64: 1e-14}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pnode_amd", "csrc")
WSPECS = ["wvpt=%d%s" % (w, st) for st in ("", ",st=0") for w in (1, 2, 4)]      # test_gpu_kernel_variants.py enumerates these
EPS = 2.0 ** -10
Q = EPS / (1.0 + EPS)                        # the one non-zero quotient of an impulse probe (un = 1, atol = 0, rtol = 1)
WORST = {}                                   # largest relative deviation from the reference seen per dtype (printed)


@pytest.fixture(autouse=True)
def _gpu():
    require_gpu()


def _const(source, name):
    with open(os.path.join(CSRC, source)) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def _vw(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def _n(n, dtype):
    return {"VW": _vw(dtype), "VW+1": _vw(dtype) + 1}.get(n, n)


def _group(dtype, d):
    """Threads that share a row (geom() in pn_rows.hip): the smallest power of two >= the row's 16-byte chunks, at most 256."""
    nch = -(-d // _vw(dtype))
    g = 1
    while g < nch and g < 256:
        g *= 2
    return g


def _dev(arr, off=0):
    """A host array on the device, `off` elements into an allocation of its own (off = 1: not 16-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    v = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)[off:]
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def _nan(n, dtype, off=0):
    v = torch.full((n + off,), float("nan"), dtype=dtype, device=DEV)[off:]
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _meets(dtype, got, want, rel, what):
    """|got - want| <= rel * want; a reference of exactly 0 (every term exactly zero) must come back as 0.0."""
    print("%s: got %.17g want %.17g" % (what, got, want))
    if want == 0.0:
        assert got == 0.0, what
        return
    dev = abs(got - want) / want
    WORST[dtype] = max(WORST.get(dtype, 0.0), dev)
    assert dev <= rel, (what, got, want, dev)


def _same(v, base):
    return v == base if base == 0.0 else v == pytest.approx(base, rel=1e-13)


# ----------------------------------------------------------------------------------------------------- B1. regimes, batch kernel
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", ["VW", "VW+1", 257, 4099])
@pytest.mark.parametrize("off", [0, 1])                      # the 16-byte form; the scalar form one element off
@pytest.mark.parametrize("write", [False, True])
def test_regimes_batch_kernel(dtype, n, off, write):
    """Default geometry and every wvpt x store policy: each meets the reference and agrees with the default to 1e-13.  write: nk = 3
    through the write path, unew bit-equal to the exact result, the norm's reference taken from the stored unew."""
    lib = _lib.load()
    n = _n(n, dtype)
    ops = HipVecOps(DEV, dtype, n)
    try:
        for name, un, err, atol, rtol in wc.cases(NP[dtype], n, dyadic=write):
            if write:
                u0, K0, ref_unew = wc.write_path_operands(NP[dtype], un, err)
                u, K, cb, ce = _dev(u0, off), [_dev(k, off) for k in K0], wc.WRITE_CB, wc.WRITE_CE
            else:
                u, K, cb, ce = _dev(un, off), [_dev(err, off)], [0.0], [1.0]
            base = None
            for spec in [None] + WSPECS:
                lib.pn_tune_set(spec.encode() if spec else None)
                unew = _nan(n, dtype, off) if write else None
                ops.combine_wrms(unew, u, K, cb, ce, atol, rtol)
                got = ops.read_enorm()
                stored = un
                if write:
                    assert np.array_equal(_bits(unew), _bits(torch.from_numpy(ref_unew))), (name, spec)
                    stored = unew.cpu().numpy()
                want = wc.wrms_ref(stored, wc.stored_uhat(stored, err), atol, rtol)
                _meets(dtype, got, want, REL[dtype], (name, spec))
                if name == "all-A1":
                    assert got == 0.0
                if base is None:
                    base = got
                assert _same(got, base), (name, spec)
    finally:
        lib.pn_tune_set(None)
    print("largest relative deviation so far: %s" % WORST)


# ------------------------------------------------------------------------------------------------------ B2. regimes, rows kernel
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [5, 24, 64, 100, 256, 512, 4099])
@pytest.mark.parametrize("write", [False, True])
def test_regimes_rows_kernel(dtype, d, write):
    """B = 7, row r is the case vector rotated by r: the reference per row; rows [B // 2:] launched alone and (d % VW == 0) the
    scalar form one element off give the same bits."""
    B, lo, vw = 7, 3, _vw(dtype)
    ops = HipVecOps(DEV, dtype, B * d)
    h = torch.ones(B, dtype=torch.float64, device=DEV)
    for name, un, err, atol, rtol in wc.cases(NP[dtype], d, dyadic=write):
        E = np.stack([np.roll(err, r) for r in range(B)])
        U = np.stack([np.roll(un, r) for r in range(B)])
        if write:
            u0, K0, ref_unew = wc.write_path_operands(NP[dtype], un, err)
            host = [np.stack([np.roll(x, r) for r in range(B)]) for x in [u0] + K0]
            ref_unew = np.stack([np.roll(ref_unew, r) for r in range(B)])
            cb, ce = wc.WRITE_CB, wc.WRITE_CE
        else:
            host, cb, ce = [U, E], [0.0], [1.0]

        def run(rows, off):
            vs = [_dev(x[rows].reshape(-1), off) for x in host]
            nb = vs[0].numel() // d
            unew = _nan(nb * d, dtype, off) if write else None
            enorm = torch.full((nb,), float("nan"), dtype=torch.float64, device=DEV)
            ops.rows_combine_wrms(nb, d, unew, vs[0], vs[1:], cb, ce, h[:nb], atol, rtol, enorm)
            return enorm, unew
        enorm, unew = run(slice(0, B), 0)
        stored = U
        if write:
            assert np.array_equal(_bits(unew.view(B, d)), _bits(torch.from_numpy(ref_unew))), name
            stored = unew.view(B, d).cpu().numpy()
        got = enorm.tolist()
        for r in range(B):
            _meets(dtype, got[r], wc.wrms_ref(stored[r], wc.stored_uhat(stored[r], E[r]), atol, rtol), REL[dtype], (name, r))
        half, _ = run(slice(lo, B), 0)
        assert np.array_equal(_bits(half), _bits(enorm[lo:])), name
        if d % vw == 0:
            scalar, sun = run(slice(0, B), 1)
            assert np.array_equal(_bits(scalar), _bits(enorm)), name
            assert not write or np.array_equal(_bits(sun), _bits(unew)), name
    print("largest relative deviation so far: %s" % WORST)


def _randn(n, dtype, seed, off=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    v = torch.randn(n + off, generator=g, dtype=dtype, device=DEV)[off:]
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def _rows_h(B):
    h = 0.05 + 0.2 * torch.rand(B, generator=torch.Generator().manual_seed(1 + B), dtype=torch.float64)
    h[::3] = 0.0
    return h.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [24, 64, 100, 256, 512])
def test_rows_stage_and_adj_theta_scalar_form_gives_the_vector_form_bits(dtype, d):
    """The header of pn_rows.hip: the scalar form walks the same chunks, so both forms give the same bits."""
    B = 7
    assert d % _vw(dtype) == 0
    ops = HipVecOps(DEV, dtype, B * d)
    h = _rows_h(B)
    src = [_randn(B * d, dtype, 100 * d + j) for j in range(4)]
    out = {}
    for off in (0, 1):
        x = [_dev(s.cpu().numpy(), off) for s in src]
        y, w, w0 = _nan(B * d, dtype, off), _nan(B * d, dtype, off), _nan(B * d, dtype, off)
        ops.rows_stage(B, d, y, x[0], x[1:], [0.3, -0.7, 1.1], h)
        ops.rows_adj_theta(B, d, w, x[0], 0.4, x[1:3], [0.3, -0.7], h)
        ops.rows_adj_theta(B, d, w0, None, 0.0, x[1:3], [0.3, -0.7], h)
        out[off] = [_bits(t) for t in (y, w, w0)]
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))


# ---------------------------------------------------------------------------------------------- B3. impulse probes, batch kernels
def _probe_positions(n, vw, cap):
    """Seams of the launch geometry: the first vectors, the end of the vector body, every tail element, lane 63 | 64 and thread
    255 | 256, the last workgroup of the first trip of a grid of `cap` workgroups, the first element of the second trip, n - 1."""
    body, trip = (n // vw) * vw, cap * 256 * vw
    want = {0, vw - 1, vw, body - 1, 63 * vw, 64 * vw, 255 * vw, 256 * vw, trip - 256 * vw, trip - 1, trip, n - 1}
    want |= set(range(body, n))
    return sorted(p for p in want if 0 <= p < n)


def _probe_size(size, dtype, cap):
    return (cap * 256 + 1) * _vw(dtype) + 3 if size == "trip+3" else _n(size, dtype)


def test_probe_positions_reach_the_seams():
    cap = _const("pn_tgrad.hip", "kTgMaxBlocks")
    for dtype in DTYPES:
        vw = _vw(dtype)
        n = _probe_size("trip+3", dtype, cap)
        assert n // vw > cap * 256 and n % vw                                   # a second trip, and a ragged tail
        pos = _probe_positions(n, vw, cap)
        assert {cap * 256 * vw - 1, cap * 256 * vw, (cap - 1) * 256 * vw, n - 1, (n // vw) * vw} <= set(pos)
        assert {0, vw - 1, vw} <= set(_probe_positions(vw + 1, vw, cap))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", ["VW+1", 4099, "trip+3"])
def test_impulse_probes_combine_wrms(dtype, size):
    """un = 1, err = 2^-10 at one position (then: everywhere but one), atol = 0, rtol = 1: the norm is q / sqrt(n) (q sqrt((n-1)/n))
    with q = 2^-10 / (1 + 2^-10), in the default geometry, with 2 and 4 vectors per thread and finished inside the launch (ticket
    hand-off and ordered_sum over the workgroup partials)."""
    lib = _lib.load()
    cap = _const("pn_tgrad.hip", "kTgMaxBlocks")
    n, vw = _probe_size(size, dtype, cap), _vw(dtype)
    ops = HipVecOps(DEV, dtype, n)
    un = torch.ones(n, dtype=dtype, device=DEV)
    err = torch.zeros(n, dtype=dtype, device=DEV)
    assert un.data_ptr() % 16 == 0 and err.data_ptr() % 16 == 0
    try:
        for fill, mark, want, rel in ((0.0, EPS, Q / math.sqrt(n), REL_ONE[dtype]), (EPS, 0.0, Q * math.sqrt((n - 1) / n), REL[dtype])):
            err.fill_(fill)
            prev = None
            for p in _probe_positions(n, vw, cap):
                if prev is not None:
                    err[prev] = fill
                err[p] = mark
                prev = p
                for spec in (None, "wvpt=2", "wvpt=4", "wfin=1"):
                    lib.pn_tune_set(spec.encode() if spec else None)
                    ops.combine_wrms(None, un, [err], [0.0], [1.0], 0.0, 1.0)
                    _meets(dtype, ops.read_enorm(), want, rel, (fill, p, spec))
    finally:
        lib.pn_tune_set(None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", ["VW+1", 4099, "trip+3"])
def test_impulse_probes_dots_and_tgrad(dtype, size):
    """pn_dots, pn_tgrad_dots and pn_rk_dense_tgrad (m = 33) on x = 3 at one position (then: everywhere but one), y = 1: sums of
    small integers are exact in double in any order, so the result is 3 (3 (n - 1)) exactly."""
    cap = _const("pn_tgrad.hip", "kTgMaxBlocks")
    n, vw, m = _probe_size(size, dtype, cap), _vw(dtype), 33
    ld = -(-n // vw) * vw
    ops = HipVecOps(DEV, dtype, n)
    x = torch.zeros(n, dtype=dtype, device=DEV)
    y = torch.ones(n, dtype=dtype, device=DEV)
    g = torch.zeros(m, ld, dtype=dtype, device=DEV)[:, :n]
    assert all(t.data_ptr() % 16 == 0 for t in (x, y, g)) and g.stride(0) % vw == 0
    coefs = [[1.0]] * m
    for fill, mark, want in ((0.0, 3.0, 3.0), (3.0, 0.0, 3.0 * (n - 1))):
        x.fill_(fill)
        g.fill_(fill)
        prev = None
        for p in _probe_positions(n, vw, cap):
            if prev is not None:
                x[prev] = fill
                g[:, prev] = fill
            x[p] = mark
            g[:, p] = mark
            prev = p
            assert ops.dots(x, [y]) == [want], (fill, p)
            acc = torch.full((3,), 0.5, dtype=torch.float64, device=DEV)
            ops.tgrad_dots(acc[1:2], [x], [y], [1.0], accumulate=False)
            assert acc.tolist() == [0.5, want, 0.5], (fill, p)
            rows = torch.full((m + 2,), 0.5, dtype=torch.float64, device=DEV)
            ops.dense_tgrad(rows[1:m + 1], g, [y], coefs, accumulate=False)
            assert rows.tolist() == [0.5] + [want] * m + [0.5], (fill, p)


# ----------------------------------------------------------------------------------- B4. impulse probes and group widths, rows
GROUPS = [1, 2, 4, 8, 16, 32, 64, 128, 256]


def _d_for(dtype, G, ragged):
    """A row length whose group is G: d % VW == 0, or ragged with the fewest chunks that still need G threads (G = 256: more chunks
    than threads, so every thread walks its chunk loop more than once)."""
    vw = _vw(dtype)
    if G == 256:
        d = 4099 if ragged else 512 * vw
    elif ragged:
        d = (G // 2 + 1) * vw - 1 if G > 1 else vw - 1
    else:
        d = G * vw
    assert _group(dtype, d) == G and (d % vw != 0) == ragged
    return d


def test_every_group_width_is_reached():
    for dtype in DTYPES:
        assert sorted({_group(dtype, _d_for(dtype, G, r)) for G in GROUPS for r in (False, True)}) == GROUPS
        assert _group(dtype, 24) == (8 if dtype == torch.float32 else 16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("ragged", [False, True])
def test_rows_impulse_probe_every_group_width(dtype, G, ragged):
    """B = d rows (at most 4099), row r carries its error in column r (r d // B): one launch probes every thread of the group,
    every slot of a chunk and every row slot of a workgroup.  Every enorm[r] is q / sqrt(d); with the error everywhere but there,
    q sqrt((d - 1) / d)."""
    d = _d_for(dtype, G, ragged)
    B = min(d, 4099)
    ops = HipVecOps(DEV, dtype, B * d)
    h = torch.ones(B, dtype=torch.float64, device=DEV)
    un = torch.ones(B * d, dtype=dtype, device=DEV)
    err = torch.zeros(B * d, dtype=dtype, device=DEV)
    rows = torch.arange(B, device=DEV)
    cols = rows * d // B
    assert int(cols[-1]) == (B - 1) * d // B and (B != d or torch.equal(cols, rows))
    for fill, mark, want, rel in ((0.0, EPS, Q / math.sqrt(d), REL_ONE[dtype]), (EPS, 0.0, Q * math.sqrt((d - 1) / d), REL[dtype])):
        err.fill_(fill)
        err.view(B, d)[rows, cols] = mark
        enorm = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
        ops.rows_combine_wrms(B, d, None, un, [err], [0.0], [1.0], h, 0.0, 1.0, enorm)
        lo, hi = float(enorm.min()), float(enorm.max())
        assert bool(torch.isfinite(enorm).all())
        _meets(dtype, lo, want, rel, (d, fill, "min"))
        _meets(dtype, hi, want, rel, (d, fill, "max"))


def _rows_tol(dtype):
    return 2e-6 if dtype == torch.float32 else 1e-14          # test_gpu_sample_adapt.py


def _rows_close(a, b, dtype):
    return torch.allclose(a.double(), b, rtol=_rows_tol(dtype), atol=_rows_tol(dtype))


def _stage_ref(B, d, u, K, coef, h):
    ref = u.double().view(B, d).clone()
    for c, k in zip(coef, K):
        ref = ref + (h.view(B, 1) * c) * k.double().view(B, d)
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("ragged", [False, True])
def test_rows_kernels_every_group_width(dtype, G, ragged):
    """rows_stage, rows_adj_theta, rows_commit and rows_adj_accum at every group width against fp64; B = 259 rows: more than one
    workgroup at every width (256 / G rows each), the last one partly live."""
    d = _d_for(dtype, G, ragged)
    B, T = 259, 3
    n = B * d
    ops = HipVecOps(DEV, dtype, n)
    u, k1, k2, k3 = [_randn(n, dtype, 1000 * d + j) for j in range(4)]
    h = _rows_h(B)
    coef = [0.3, -0.7, 1.1]
    y = _nan(n, dtype)
    ops.rows_stage(B, d, y, u, [k1, k2, k3], coef, h)
    assert _rows_close(y.view(B, d), _stage_ref(B, d, u, [k1, k2, k3], coef, h), dtype)
    one = HipVecOps(DEV, dtype, d)
    for r in (0, 1, B // 2, B - 1):                                            # a row is the bits of pn_rk_stage with the same h
        yr = torch.empty(d, dtype=dtype, device=DEV)
        one.rk_stage(yr, u.view(B, d)[r].clone(), [k.view(B, d)[r].clone() for k in (k1, k2, k3)], [float(h[r]) * c for c in coef])
        assert torch.equal(yr, y.view(B, d)[r]), r
    w = _nan(n, dtype)
    ops.rows_adj_theta(B, d, w, u, 0.4, [k1, k2], [0.3, -0.7], h)
    hb = h.view(B, 1)
    ref = (hb * 0.4) * u.double().view(B, d) + (hb * 0.3) * k1.double().view(B, d) + (hb * -0.7) * k2.double().view(B, d)
    assert _rows_close(w.view(B, d), ref, dtype)
    gen = torch.Generator().manual_seed(B + d)
    acc = torch.randint(0, 2, (B,), generator=gen).to(torch.int32).to(DEV)
    hit = (torch.randint(0, T + 1, (B,), generator=gen) - 1).to(torch.int32).to(DEV)
    assert 0 < int(acc.sum()) < B and int((hit < 0).sum()) > 0 and int((hit >= 0).sum()) > 0
    sol = torch.zeros(T, n, dtype=dtype, device=DEV)
    nxt = _nan(n, dtype)
    ops.rows_commit(B, d, nxt, u, k1, acc, hit, sol, n, T)
    a = acc.bool().view(B, 1)
    assert torch.equal(nxt.view(B, d), torch.where(a, k1.view(B, d), u.view(B, d)))
    want = torch.zeros(T, B, d, dtype=dtype, device=DEV)
    for i in range(T):
        want[i] = torch.where((a.view(B) & (hit == i)).view(B, 1), k1.view(B, d), want[i])
    assert torch.equal(sol.view(T, B, d), want)
    gg = torch.stack([_randn(n, dtype, 2000 * d + i) for i in range(T)])
    out = _nan(n, dtype)
    ops.rows_adj_accum(B, d, out, u, [k1, k2], gg, gg.stride(0), hit, T)
    ref = u.double().view(B, d) + k1.double().view(B, d) + k2.double().view(B, d)
    for i in range(T):
        ref = ref + torch.where((hit == i).view(B, 1), gg[i].double().view(B, d), torch.zeros_like(ref))
    assert _rows_close(out.view(B, d), ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 8, 64])
def test_rows_second_trip_with_a_partly_live_last_workgroup(dtype, G):
    """B = kRowsMaxBlocks * (256 / G) + 5 rows of the smallest d whose group is G: every workgroup takes a second trip of its
    block-stride loop, and on it five rows are left: the last workgroup with any is partly live.  rows_combine_wrms and rows_stage on random data,
    and the impulse probe on the last five rows (all other rows: exactly 0)."""
    vw = _vw(dtype)
    cap = _const("pn_rows.hip", "kRowsMaxBlocks")
    d = (G // 2) * vw + 1
    assert _group(dtype, d) == G and _group(dtype, d - 1) < G or G == 1
    rpb = 256 // G
    B = cap * rpb + 5
    assert B - cap * rpb == 5 and 5 % rpb != 0 and B * d <= 5 * 10 ** 6      # second trip: five rows, its last workgroup partly live
    n = B * d
    ops = HipVecOps(DEV, dtype, n)
    ones = torch.ones(B, dtype=torch.float64, device=DEV)
    u, k = _randn(n, dtype, 7 * d), _randn(n, dtype, 7 * d + 1) * 1e-3
    atol, rtol = 1e-5, 1e-4
    enorm = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    ops.rows_combine_wrms(B, d, None, u, [k], [0.0], [1.0], ones, atol, rtol, enorm)
    un, uh = u.double().view(B, d), (u + k).double().view(B, d)                   # u + k: one rounding in the storage type
    ref = ((((un - uh) / (atol + rtol * torch.maximum(un.abs(), uh.abs()))) ** 2).sum(1) / d).sqrt()
    some = ref > 0                                                                # a row whose uhat == u everywhere: exactly 0
    dev = float(((enorm - ref).abs()[some] / ref[some]).max())
    print("second trip, G = %d: largest relative deviation %.3g" % (G, dev))
    assert dev <= REL[dtype] and bool((enorm[~some] == 0.0).all()) and int(some.sum()) > B // 2
    h = _rows_h(B)
    y = _nan(n, dtype)
    ops.rows_stage(B, d, y, u, [k], [0.3], h)
    assert _rows_close(y.view(B, d), _stage_ref(B, d, u, [k], [0.3], h), dtype)
    un1 = torch.ones(n, dtype=dtype, device=DEV)
    err = torch.zeros(n, dtype=dtype, device=DEV)
    last = torch.arange(B - 5, B, device=DEV)
    err.view(B, d)[last, last % d] = EPS
    enorm.fill_(float("nan"))
    ops.rows_combine_wrms(B, d, None, un1, [err], [0.0], [1.0], ones, 0.0, 1.0, enorm)
    assert bool((enorm[:B - 5] == 0.0).all())
    for r, v in enumerate(enorm[B - 5:].tolist()):
        _meets(dtype, v, Q / math.sqrt(d), REL_ONE[dtype], (G, "last rows", r))


# --------------------------------------------------------------------------------------------------------------- B5. end to end
def test_device_solve_equals_the_cpu_stand_in_at_group_width_16():
    """test_gpu_sample_adapt.py::test_device_solve_equals_the_cpu_stand_in with the spiral lifted to d = 24 by block-diagonal
    repetition (twelve spirals per row): a real per-sample solve with 16 threads per row (fp64: 12 chunks)."""
    from _cpu_rows_ops import CpuRowsOps
    from test_gpu_sample_adapt import _rel, _solve, _spread
    assert _group(torch.float64, 24) == 16
    y0 = _spread(6 * 12).reshape(6, 24)
    sol, gu, gp, ode = _solve(y0, DEV, "5dp", 1e-8)
    rsol, rgu, rgp, rode = _solve(y0, torch.device("cpu"), "5dp", 1e-8, backend=CpuRowsOps)
    assert sol.shape[1:] == (6, 24)
    assert torch.equal(ode.sample_steps, rode.sample_steps) and torch.equal(ode.sample_rejections, rode.sample_rejections)
    assert ode.rounds == rode.rounds and int(ode.sample_steps.max()) >= 2 * int(ode.sample_steps.min())
    worst = max(_rel(sol, rsol), _rel(gu, rgu), _rel(gp, rgp))
    print("sample mode, d = 24: device against the CPU stand-in %.2e" % worst)
    assert worst <= 1e-11
