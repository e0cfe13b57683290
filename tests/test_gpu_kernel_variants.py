"""-m gpu: the compiled forms of the streaming kernels that no other kernel test reaches, each against plain fp64 host arithmetic.

A. the 16-byte form of pn_rk_dense_eval / pn_rk_dense_adjoint (csrc/pn_dense.hip): ragged tails, padded row strides, more vectors
   than the capped grid covers in one trip, every nk / nd, both store policies -- against fp64, and bit for bit against the
   scalar form of the same template on the same values one element off.
B. both reductions of csrc/pn_tgrad.hip on vectors longer than one trip of their capped grid.
C. every geometry PN_TUNE / pn_tune_set can select in csrc/pn_kernels.hip: the result is the default geometry's, bit for bit.
D. every NK of the pn_rows_* kernels (csrc/pn_rows.hip), and a NaN / inf row that must not reach the other rows' norms.

Every test that aims at one form asserts, in Python, the predicate the launcher uses to choose it (data_ptr() % 16, row stride % VW,
n % VW), so a layout mistake cannot move the test onto the other form unnoticed.  Inputs are drawn on the device (the largest
cases hold 10^8 numbers) and copied back for the reference."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import require_gpu
from oracle import ts_oracle
from pnode_amd import _lib
from pnode_amd._vecops import HipVecOps

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
SENT = -7.0                      # what lies around and between the rows of every buffer; must come back unchanged
GUARD = 8                        # sentinel elements behind every buffer
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pnode_amd", "csrc")


@pytest.fixture(autouse=True)
def _gpu():
    require_gpu()


def _const(source, name):
    """`constexpr int <name> = <value>;` of a kernel file: the sizes below are chosen against the launchers' own grid caps."""
    with open(os.path.join(CSRC, source)) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def _vw(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def _size(n, dtype):
    return {"VW": _vw(dtype), "VW+1": _vw(dtype) + 1}.get(n, n)


def _randn(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=dtype, device=DEV)


def _place(values, off, ld=None):
    """`values` (n, or m rows of n) in an allocation of their own: `off` sentinel elements, the rows with stride `ld` (sentinels
    between them), GUARD sentinels.  Returns (storage, view of the values)."""
    two = values.dim() == 2
    m, n = (values.shape if two else (1, values.numel()))
    ld = n if ld is None else ld
    st = torch.full((off + m * ld + GUARD,), SENT, dtype=values.dtype, device=DEV)
    body = st[off: off + m * ld].view(m, ld)
    body[:, :n] = values.view(m, n)
    view = body[:, :n] if two else st[off: off + n]
    if two:
        assert view.stride(0) == ld
    return st, view


def _surroundings_untouched(st, off, m, n, ld=None):
    ld = n if ld is None else ld
    body = st[off: off + m * ld].view(m, ld)
    return bool((st[:off] == SENT).all()) and bool((st[off + m * ld:] == SENT).all()) and bool((body[:, n:] == SENT).all())


def _vector_form(dtype, tensors, ld=None):
    """What dense_eval / dense_adjoint / dense_tgrad (and al16 everywhere) compute before they pick the 16-byte form."""
    return all(t.data_ptr() % 16 == 0 for t in tensors) and (ld is None or ld % _vw(dtype) == 0)


def _maxdiff(a, ref):
    """max |a - ref| with the comparison on the device (ref: fp64 host tensor); NaN if any entry of `a` is NaN."""
    return float((a.double() - ref.to(DEV)).abs().max())


# ------------------------------------------------------------------------------------------------ A. dense kernels, 16-byte form
# (n, m, nk or nd, pad): pad = further vector widths of row stride beyond ceil(n / VW) * VW
_SMALL = [(n, m, 1 + m % 7, 0) for n in ("VW", "VW+1", 4097, 4099) for m in (1, 4, 5, 32, 33, 65)]
_DISPATCH_NK = [(4099, 5, nk, 0) for nk in range(1, 8)]
_DISPATCH_ND = [(4099, 5, nd, 0) for nd in range(0, 8)]
_PADDED = [(4099, 5, 4, 1), (2 ** 21, 4, 2, 1)]
# 2**21: C3a, for fp32 exactly the capped grid; 2**22 + 3: twice the capped grid (fp32) and a tail.  m = 65 stays at n <= 4099.
_LARGE = [(2 ** 21, 33, 7, 0), (2 ** 22 + 3, 1, 1, 0), (2 ** 22 + 3, 5, 3, 0)]


def _dense_setup(dtype, n, m, pad):
    vw = _vw(dtype)
    n = _size(n, dtype)
    ld = -(-n // vw) * vw + pad * vw
    return vw, n, ld


def _second_trip(dtype, n):
    return n // _vw(dtype) > _const("pn_dense.hip", "kDenseMaxBlocks") * 256


def test_dense_sizes_reach_the_capped_grid_and_pass_it():
    assert 2 ** 21 // 4 == _const("pn_dense.hip", "kDenseMaxBlocks") * 256               # fp32: exactly the cap, one trip
    assert not _second_trip(torch.float32, 2 ** 21) and _second_trip(torch.float64, 2 ** 21)
    assert _second_trip(torch.float32, 2 ** 22 + 3) and (2 ** 22 + 3) % 4 and (2 ** 22 + 3) % 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,nk,pad", _SMALL + _DISPATCH_NK + _PADDED + _LARGE)
def test_dense_eval_16_byte_form(dtype, n, m, nk, pad):
    """out_o = u + sum_j c_oj K_j in the VW = 4 / VW = 2 instantiation: against fp64 with the coefficients rounded once to the
    storage type (the tolerances of test_gpu_dense_output.py), the same bits as the scalar form on the same values one element
    off, the same bits on a second launch, with plain and with non-temporal stores; sentinels around and between the rows stay."""
    vw, n, ld = _dense_setup(dtype, n, m, pad)
    ops = HipVecOps(DEV, dtype, n)
    u = _randn(n, dtype, n * 7 + m)
    K = _randn((nk, n), dtype, n * 7 + m + 1)
    coefs = torch.randn(m, nk, generator=torch.Generator().manual_seed(n + m), dtype=torch.float64) * 0.1
    cq = coefs.to(dtype).double()
    ref = u.double().cpu()[None, :] + cq @ K.double().cpu()
    tol = (1e-5 if dtype == torch.float32 else 1e-13) * float(ref.abs().max())
    nan_rows = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    for flags in (0, _lib.PN_DENSE_NONTEMPORAL):
        ops.dense_flags = flags
        res = {}
        for off in (0, 1):
            ust, uv = _place(u, off)
            kst = [_place(K[j], off) for j in range(nk)]
            Kv = [v for _, v in kst]
            ost, out = _place(nan_rows, off, ld)
            assert _vector_form(dtype, [uv, out] + Kv, out.stride(0)) == (off == 0)
            assert (n % vw != 0) == (n not in (vw, 2 ** 21))                   # every other size runs the ragged tail
            ops.dense_eval(out, uv, Kv, coefs.tolist())
            res[off] = out.clone()
            assert _surroundings_untouched(ost, off, m, n, ld), (flags, off)
            assert _surroundings_untouched(ust, off, 1, n) and torch.equal(uv, u)
            assert all(_surroundings_untouched(s, off, 1, n) and torch.equal(v, K[j]) for j, (s, v) in enumerate(kst))
            _, again = _place(nan_rows, off, ld)
            ops.dense_eval(again, uv, Kv, coefs.tolist())
            assert torch.equal(again, res[off]), (flags, off)
        d = _maxdiff(res[0], ref)
        assert d <= tol, (flags, d, tol)
        assert torch.equal(res[0], res[1]), flags                             # 16-byte form == scalar form, bit for bit
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,m,nd,pad", _SMALL + _DISPATCH_ND + _PADDED + _LARGE)
def test_dense_adjoint_16_byte_form(dtype, n, m, nd, pad):
    """D_j (+)= sum_o c_oj g_o, G (+)= sum_o g_o in the VW = 4 / VW = 2 instantiation, with and without G (nd = 0: G alone),
    overwriting NaN-filled outputs (accumulate = 0, also when m > 32 makes later chunks continue the first) and adding to given
    ones (accumulate = 1): against fp64, bit for bit against the scalar form one element off, bit for bit on a second launch."""
    vw, n, ld = _dense_setup(dtype, n, m, pad)
    ops = HipVecOps(DEV, dtype, n)
    g = _randn((m, n), dtype, n * 11 + m)
    D0 = _randn((max(nd, 1), n), dtype, n * 11 + m + 1)
    G0 = _randn(n, dtype, n * 11 + m + 2)
    coefs = torch.randn(m, nd, generator=torch.Generator().manual_seed(n + m + 1), dtype=torch.float64) * 0.1
    cq = coefs.to(dtype).double()
    gd = g.double().cpu()
    refD, refG = cq.t() @ gd, gd.sum(0)
    tol = (1e-5 if dtype == torch.float32 else 1e-13) * math.sqrt(m)
    nan_vec = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
    for with_g in (True, False):
        for acc in (0, 1):
            if nd == 0 and not with_g:
                continue                                                       # nothing to compute: the entry point refuses it
            res = {}
            for off in (0, 1):
                gst, gv = _place(g, off, ld)

                def outputs():
                    ds = [_place(D0[j] if acc else nan_vec, off) for j in range(nd)]
                    gb = _place(G0 if acc else nan_vec, off) if with_g else (None, None)
                    return ds, gb
                ds, gb = outputs()
                Dv = [v for _, v in ds]
                assert _vector_form(dtype, [gv] + Dv + ([gb[1]] if with_g else []), gv.stride(0)) == (off == 0)
                ops.dense_adjoint(Dv, gb[1], gv, coefs.tolist(), accumulate=bool(acc))
                res[off] = [v.clone() for v in Dv] + ([gb[1].clone()] if with_g else [])
                assert all(_surroundings_untouched(s, off, 1, n) for s, _ in ds + ([gb] if with_g else [])), (with_g, acc, off)
                assert _surroundings_untouched(gst, off, m, n, ld) and torch.equal(gv, g)
                ds2, gb2 = outputs()
                ops.dense_adjoint([v for _, v in ds2], gb2[1], gv, coefs.tolist(), accumulate=bool(acc))
                second = [v for _, v in ds2] + ([gb2[1]] if with_g else [])
                assert all(torch.equal(a, b) for a, b in zip(second, res[off])), (with_g, acc, off)
            if nd:
                want = refD + (D0[:nd].double().cpu() if acc else 0)
                d = _maxdiff(torch.stack(res[0][:nd]), want)
                assert d <= tol * max(float(want.abs().max()), 1.0), (with_g, acc, d)
            if with_g:
                want = refG + (G0.double().cpu() if acc else 0)
                d = _maxdiff(res[0][nd], want)
                assert d <= tol * max(float(want.abs().max()), 1.0), (with_g, acc, d)
            assert all(torch.equal(a, b) for a, b in zip(res[0], res[1])), (with_g, acc)      # 16-byte form == scalar form
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ B. tgrad, vector form past the grid cap
def _aligned_rows(count, n, dtype, seed):
    """`count` vectors of n elements in one allocation, every row on a 16-byte boundary, row stride a multiple of VW (the layout
    of _rows(misaligned=False) in test_gpu_time_grads.py)."""
    vw = _vw(dtype)
    ld = -(-n // vw) * vw
    rows = _randn(count * ld, dtype, seed).view(count, ld)[:, :n]
    assert all(r.data_ptr() % 16 == 0 for r in rows) and rows.stride(0) % vw == 0
    return rows


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [2 ** 21, 2 ** 21 + 3])
def test_tgrad_vector_form_past_the_grid_cap(dtype, n):
    """Both reductions where the 16-byte form's grid-stride loop takes a second trip (fp32: 2**19 vectors on 1024 workgroups of
    256 threads), with and without the ragged tail: fp64 host sums within 1e-12 max(1, |ref|) sqrt(n), neighbouring slots
    untouched, bitwise equal run to run, accumulate adds exactly once."""
    vw = _vw(dtype)
    assert n // vw > _const("pn_tgrad.hip", "kTgMaxBlocks") * 256 and (n % vw != 0) == (n != 2 ** 21)
    ops = HipVecOps(DEV, dtype, n)
    for np_ in (1, 7):
        rows = _aligned_rows(2 * np_, n, dtype, n + np_)
        xs, ys = [rows[p] for p in range(np_)], [rows[np_ + p] for p in range(np_)]
        cs = torch.randn(np_, generator=torch.Generator().manual_seed(np_), dtype=torch.float64).tolist()
        dot = sum(c * float(x.double().cpu() @ y.double().cpu()) for c, x, y in zip(cs, xs, ys))
        plain = torch.full((3,), 0.5, dtype=torch.float64, device=DEV)
        ops.tgrad_dots(plain[1:2], xs, ys, cs, accumulate=False)
        assert abs(float(plain[1]) - dot) <= 1e-12 * max(1.0, abs(dot)) * (n ** 0.5)
        assert float(plain[0]) == 0.5 and float(plain[2]) == 0.5
        acc = torch.full((3,), 0.5, dtype=torch.float64, device=DEV)
        ops.tgrad_dots(acc[1:2], xs, ys, cs, accumulate=True)
        assert abs(float(acc[1]) - (0.5 + dot)) <= 1e-12 * max(1.0, abs(0.5 + dot)) * (n ** 0.5)
        assert float(acc[0]) == 0.5 and float(acc[2]) == 0.5
        assert float(acc[1]) == 0.5 + float(plain[1])                        # one fp64 addition of the same total: exactly once
        again = torch.full((3,), 0.5, dtype=torch.float64, device=DEV)
        ops.tgrad_dots(again[1:2], xs, ys, cs, accumulate=True)
        assert torch.equal(again, acc)
    for m, nk in ((1, 1), (32, 7), (33, 6)):
        gr = _aligned_rows(m, n, dtype, n + 100 + m)
        kr = _aligned_rows(nk, n, dtype, n + 200 + m)
        Ks = [kr[j] for j in range(nk)]
        assert _vector_form(dtype, [gr] + Ks, gr.stride(0))
        co = torch.randn(m, nk, generator=torch.Generator().manual_seed(m), dtype=torch.float64)
        ref = ((gr.double().cpu() @ kr.double().cpu().t()) * co).sum(1)
        bound = 1e-12 * max(1.0, float(ref.abs().max())) * (n ** 0.5)
        plain = torch.zeros(m + 2, dtype=torch.float64, device=DEV)
        ops.dense_tgrad(plain[1:m + 1], gr, Ks, co.tolist(), accumulate=False)
        a = plain.cpu()
        assert float(a[0]) == 0.0 and float(a[m + 1]) == 0.0
        assert float((a[1:m + 1] - ref).abs().max()) <= bound
        start = torch.randn(m + 2, generator=torch.Generator().manual_seed(m + 1), dtype=torch.float64)
        b = start.to(DEV)
        ops.dense_tgrad(b[1:m + 1], gr, Ks, co.tolist(), accumulate=True)
        c = start.to(DEV)
        ops.dense_tgrad(c[1:m + 1], gr, Ks, co.tolist(), accumulate=True)
        assert torch.equal(b, c)
        assert torch.equal(b.cpu()[1:m + 1], start[1:m + 1] + a[1:m + 1])    # one fp64 addition per slot
        assert float(b[0]) == float(start[0]) and float(b[m + 1]) == float(start[m + 1])
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- C. tuned variants
def _tol(dtype):
    return 2e-6 if dtype == torch.float32 else 1e-14


def _launcher_source():
    with open(os.path.join(CSRC, "pn_kernels.hip")) as fh:
        return fh.read()


def _geo_list():
    """Every (vpt, ld, st) of the launcher's PN_GEO list."""
    return sorted({tuple(int(x) for x in t) for t in re.findall(r"PN_GEO\((\d), (\d), (\d)\)", _launcher_source())})


GEO = _geo_list()
GEO_SPECS = ["vpt=%d,ld=%d,st=%d" % t for t in GEO]
BLOCK_SPECS = ["block=%d,vpt=%d" % (b, v) for b in (512, 1024) for v in (1, 2)]
CAP_SPECS = ["cap=1", "cap=7", "cap=64", "cap=7,vpt=4", "cap=64,vpt=4", "cap=7,block=512,vpt=2"]
XCD_SPECS = ["xcd=1", "xcd=1,vpt=1", "xcd=1,vpt=2", "xcd=1,vpt=4"]
# elements: ragged with fewer than 8 workgroups; ragged with a workgroup count that is no multiple of 8; ragged and large enough
# that every cap leaves a partial last trip; the 4096 x 512 state
LIN_SIZES = [1027, 13317, 1000003, 4096 * 512]


def test_the_geometry_list_is_the_one_this_file_was_written_for():
    assert len(GEO) == 15 and (2, 0, 2) in GEO and (2, 1, 2) in GEO and (4, 0, 1) in GEO


def _spec_geometry(spec, nvec):
    kv = dict(item.split("=") for item in spec.split(",") if item)
    vpt = int(kv.get("vpt", 0)) or (1 if nvec < 256 * 256 * 8 else 2)
    per = int(kv.get("block", 256)) * vpt
    return per, -(-nvec // per), int(kv.get("cap", 0))


def _vectors(k, n, dtype, seed):
    """k vectors of n elements, each on a 16-byte boundary (rows of a matrix whose stride is a multiple of VW)."""
    vw = _vw(dtype)
    vs = [r[:n] for r in _randn((k, -(-n // vw) * vw), dtype, seed)]
    assert all(v.data_ptr() % 16 == 0 and v.is_contiguous() for v in vs)
    return vs


def _lin_inputs(dtype, n):
    return _vectors(9, n, dtype, n * 7 + 9)


def _lin_family(ops, dtype, n, x, fill=float("nan")):
    """The operations of the pn_lincomb_kernel family on the vectors x[0..8]; returns {name: tuple of outputs}."""
    out = {}
    new = lambda: torch.full((n,), fill, dtype=dtype, device=DEV)   # noqa: E731
    for nk in (1, 6):
        y = new()
        ops.rk_stage(y, x[0], x[1:1 + nk], [0.3 * (j + 1) * (-1) ** j for j in range(nk)])
        out["rk_stage nk=%d" % nk] = (y,)
    for lam in (x[0], None):
        w = new()
        ops.adj_theta(w, lam, 0.125, x[1:4], [0.2, -0.4, 0.7])
        out["adj_theta lambda=%s" % (lam is not None)] = (w,)
    lam, wn = x[0].clone(), new()
    ops.adj_accum(lam, lam, x[2:6], [1.0, 0.0025, 1.0, -0.5], x[1], wn, 0.0025)           # in place, fused second output
    out["adj_accum"] = (lam, wn)
    o = new()
    ops.lincomb(o, x[:8], [0.5, -0.25, 0.125, 1.5, -1.0, 0.75, 0.1, -0.3])
    out["lincomb 8"] = (o,)
    assert all(t.data_ptr() % 16 == 0 for ts in out.values() for t in ts) and all(v.data_ptr() % 16 == 0 for v in x)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", LIN_SIZES)
def test_lincomb_family_default_geometry_against_fp64(dtype, n):
    ops = HipVecOps(DEV, dtype, n)
    x = _lin_inputs(dtype, n)
    got = _lin_family(ops, dtype, n, x)
    X = [v.double().cpu() for v in x]
    ref = {}
    for nk in (1, 6):
        ref["rk_stage nk=%d" % nk] = (X[0] + sum(0.3 * (j + 1) * (-1) ** j * X[1 + j] for j in range(nk)),)
    th = sum(c * v for c, v in zip([0.2, -0.4, 0.7], X[1:4]))
    ref["adj_theta lambda=True"] = (0.125 * X[0] + th,)
    ref["adj_theta lambda=False"] = (th,)
    lam = X[0] + sum(c * v for c, v in zip([1.0, 0.0025, 1.0, -0.5], X[2:6])) + X[1]
    ref["adj_accum"] = (lam, 0.0025 * lam)
    ref["lincomb 8"] = (sum(c * v for c, v in zip([0.5, -0.25, 0.125, 1.5, -1.0, 0.75, 0.1, -0.3], X[:8])),)
    assert set(ref) == set(got)
    for name in ref:
        for a, b in zip(got[name], ref[name]):
            assert torch.allclose(a.double().cpu(), b, rtol=_tol(dtype), atol=_tol(dtype)), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", LIN_SIZES)
@pytest.mark.parametrize("spec", GEO_SPECS + BLOCK_SPECS + CAP_SPECS + XCD_SPECS)
def test_lincomb_family_variant_gives_the_default_bits(dtype, n, spec):
    """Per element every geometry does the same arithmetic: a remap that skips or doubles a tile, a grid-stride loop that drops
    its last partial trip, or a store with a wrong operand shows as a difference (skipped elements keep their NaN fill)."""
    lib = _lib.load()
    ops = HipVecOps(DEV, dtype, n)
    x = _lin_inputs(dtype, n)
    nvec = n // _vw(dtype)
    per, nb, cap = _spec_geometry(spec, nvec)
    if n == 1027:
        assert _spec_geometry("", nvec)[1] < 8 and n % _vw(dtype)
    if n == 13317:
        assert _spec_geometry("", nvec)[1] > 8 and _spec_geometry("", nvec)[1] % 8 and n % _vw(dtype)
    if n == 1000003:
        assert _spec_geometry("", nvec)[1] % 8 and n % _vw(dtype)
        if cap:
            assert nb > cap and nvec % (cap * per) != 0                        # several trips, the last one partial
    base = _lin_family(ops, dtype, n, x)
    try:
        lib.pn_tune_set(spec.encode())
        got = _lin_family(ops, dtype, n, x)
    finally:
        lib.pn_tune_set(None)
    torch.cuda.synchronize()
    for name in base:
        for a, b in zip(got[name], base[name]):
            assert torch.equal(a, b), (spec, name, int((a != b).sum()))
    after = _lin_family(ops, dtype, n, x)                                      # and the default is back
    assert all(torch.equal(a, b) for name in base for a, b in zip(after[name], base[name]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spec", ["block=512,vpt=4", "block=1024,vpt=1,st=0", "vpt=3", "vpt=4,ld=1", "vpt=1,st=2"])
def test_a_refused_geometry_raises_and_writes_nothing(dtype, spec):
    lib = _lib.load()
    n = 13317
    ops = HipVecOps(DEV, dtype, n)
    x = _lin_inputs(dtype, n)
    y = torch.full((n,), SENT, dtype=dtype, device=DEV)
    assert y.data_ptr() % 16 == 0                                              # the geometry list is consulted on the 16-byte path
    try:
        lib.pn_tune_set(spec.encode())
        with pytest.raises(_lib.PnError, match="PN_TUNE"):
            ops.rk_stage(y, x[0], x[1:3], [0.5, -0.25])
    finally:
        lib.pn_tune_set(None)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
    ops.rk_stage(y, x[0], x[1:3], [0.5, -0.25])
    ref = x[0].double() + 0.5 * x[1].double() - 0.25 * x[2].double()
    assert torch.allclose(y.double(), ref, rtol=_tol(dtype), atol=_tol(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", LIN_SIZES)
@pytest.mark.parametrize("nk", [1, 7])
def test_combine_wrms_store_policy_and_vectors_per_thread(dtype, n, nk):
    """st=0 (plain stores) and the default (non-temporal) crossed with wvpt 1 | 2 | 4: unew has the same bits in all of them,
    the norms agree to round-off of the double sum (rel 1e-13, the figure of the reproducibility test in test_gpu_kernels.py);
    unew against fp64 as in test_combine_wrms."""
    lib = _lib.load()
    ops = HipVecOps(DEV, dtype, n)
    x = _lin_inputs(dtype, n)
    u, K = x[0], x[1:1 + nk]
    cb = [0.01 * (j + 1) for j in range(nk)]
    ce = [1e-4 * (-1) ** j * (j + 1) for j in range(nk)]
    assert all(v.data_ptr() % 16 == 0 for v in x)

    def run():
        unew = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
        assert unew.data_ptr() % 16 == 0
        ops.combine_wrms(unew, u, K, cb, ce, 1e-4, 1e-4)
        return unew, ops.read_enorm()
    base_u, base_v = run()
    ref = u.double().cpu() + sum(c * k.double().cpu() for c, k in zip(cb, K))
    assert torch.allclose(base_u.double().cpu(), ref, rtol=4 * _tol(dtype), atol=4 * _tol(dtype))
    assert math.isfinite(base_v) and base_v > 0
    # the norm against fp64 from the STORED unew and the stored uhat (err as the kernel's fma chain forms it: fp32 products are
    # exact in fp64, one rounding per step): what is left for fp32 states is the rounding of tol and of the quotient, 5e-7
    npd = np.float32 if dtype == torch.float32 else np.float64
    un = base_u.cpu().numpy()
    err = np.zeros(n, dtype=npd)
    for c, k in zip(ce, K):
        err = (np.float64(npd(c)) * k.cpu().numpy().astype(np.float64) + err.astype(np.float64)).astype(npd)
    want = ts_oracle.wrms(un, (un + err).astype(npd), 1e-4, 1e-4)
    assert base_v == pytest.approx(want, rel=1e-6 if dtype == torch.float32 else 1e-9)
    try:
        for st in ("", ",st=0"):
            for wvpt in (1, 2, 4):
                spec = "wvpt=%d%s" % (wvpt, st)
                lib.pn_tune_set(spec.encode())
                un, v = run()
                assert torch.equal(un, base_u), spec
                assert v == pytest.approx(base_v, rel=1e-13), spec
    finally:
        lib.pn_tune_set(None)


def _pvec_values():
    """The values of pvec= that select a compiled form of pn_param_accum_multi: the default and what the launcher compares with."""
    return sorted({1} | {int(v) for v in re.findall(r"tune\(\)\.pvec == (\d+)", _launcher_source())})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nsets", [3, 20])                  # 20: more live sources than one chunk of 16 loads
def test_param_accum_multi_variants(dtype, nsets):
    """pvec (vectors per thread) x pnt (non-temporal loads): the bits of the default, and of successive pn_param_accum launches;
    ragged lengths, odd offsets (the scalar branch of a workgroup) and missing gradients included."""
    lib = _lib.load()
    assert _pvec_values() == [1, 2]
    lens = [1, 100, 50, 7, 512 * 512, 3, 0, 1025, 2048 + 4, 4096] + [5] * 12
    ops = HipVecOps(DEV, dtype, 8)
    offs, off = [], 0
    for ln in lens:
        offs.append(off)
        off += ln
    mu0 = _randn(off, dtype, 7)
    sets, alphas = [], []
    for j in range(nsets):
        sets.append([_randn(ln, dtype, 100 * j + i) if ln and (i + j) % 5 != 3 else None for i, ln in enumerate(lens)])
        alphas.append(0.25 * (j + 1) * (-1) ** j)
    sets[0][4] = None
    one = mu0.clone()
    for a, gs in zip(alphas, sets):
        ops.param_accum(one, a, gs, offs, lens)
    base = mu0.clone()
    ops.param_accum_multi(base, alphas, sets, offs, lens)
    assert torch.equal(base, one)
    ref = mu0.double().cpu()
    for a, gs in zip(alphas, sets):
        for gr, o, ln in zip(gs, offs, lens):
            if gr is not None:
                ref[o:o + ln] += a * gr.double().cpu()
    scale = 10 * _tol(dtype) * nsets
    assert torch.allclose(base.double().cpu(), ref, rtol=scale, atol=scale)
    try:
        for pvec in _pvec_values():
            for pnt in (0, 1):
                spec = "pvec=%d,pnt=%d" % (pvec, pnt)
                lib.pn_tune_set(spec.encode())
                got = mu0.clone()
                ops.param_accum_multi(got, alphas, sets, offs, lens)
                assert torch.equal(got, base), (spec, int((got != base).sum()))
    finally:
        lib.pn_tune_set(None)


# -------------------------------------------------------------------------------------------------------------- D. rows kernels
ROWS_SHAPES = [(300, 512), (37, 4099)]          # aligned: the 16-byte form; ragged: the scalar form of the same kernels


def _rows_tol(dtype):
    return 2e-6 if dtype == torch.float32 else 1e-14          # test_gpu_sample_adapt.py


def _rows_close(a, b, dtype):
    return torch.allclose(a.double(), b, rtol=_rows_tol(dtype), atol=_rows_tol(dtype))


def _rows_vecs(B, d, dtype, k, seed=0):
    return _vectors(k, B * d, dtype, B * 131 + d * 7 + k + seed)


def _rows_h(B, zeros=True):
    h = 0.05 + 0.2 * torch.rand(B, generator=torch.Generator().manual_seed(1 + B), dtype=torch.float64)
    if zeros:
        h[::3] = 0.0
    return h.to(DEV)


def _rows_form(dtype, B, d, tensors):
    """rows_lin / rows_combine / rows_accum: the 16-byte form needs d % VW == 0 and every base on a 16-byte boundary."""
    vec = d % _vw(dtype) == 0 and all(t.data_ptr() % 16 == 0 for t in tensors)
    assert vec == ((B, d) == ROWS_SHAPES[0])
    return vec


def _group(dtype, d):
    """Threads that share a row (geom() in pn_rows.hip): the smallest power of two >= the row's 16-byte chunks, at most 256."""
    nch = -(-d // _vw(dtype))
    g = 1
    while g < nch and g < 256:
        g *= 2
    return g


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,d", ROWS_SHAPES)
@pytest.mark.parametrize("nk", range(1, 8))
def test_rows_stage_every_nk(dtype, B, d, nk):
    ops = HipVecOps(DEV, dtype, B * d)
    u, *K = _rows_vecs(B, d, dtype, nk + 1)
    h = _rows_h(B)
    coef = [0.3 * (j + 1) * (-1) ** j for j in range(nk)]
    y = torch.full((B * d,), float("nan"), dtype=dtype, device=DEV)
    _rows_form(dtype, B, d, [y, u] + K)
    ops.rows_stage(B, d, y, u, K, coef, h)
    hb = h.view(B, 1)
    ref = u.double().view(B, d).clone()
    for c, k in zip(coef, K):
        ref = ref + (hb * c) * k.double().view(B, d)
    assert _rows_close(y.view(B, d), ref, dtype)
    assert torch.equal(y.view(B, d)[0], u.view(B, d)[0])                      # h = 0: the state, bit for bit
    one = HipVecOps(DEV, dtype, d)
    for r in sorted({0, 1, B // 2, B - 1}):                                   # a row is the bits of pn_rk_stage with the same h
        yr = torch.empty(d, dtype=dtype, device=DEV)
        hr = float(h[r])
        one.rk_stage(yr, u.view(B, d)[r].clone(), [k.view(B, d)[r].clone() for k in K], [hr * c for c in coef])
        assert torch.equal(yr, y.view(B, d)[r]), r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,d", ROWS_SHAPES)
@pytest.mark.parametrize("nk", range(1, 8))
def test_rows_combine_wrms_every_nk(dtype, B, d, nk):
    ops = HipVecOps(DEV, dtype, B * d)
    u, *K = _rows_vecs(B, d, dtype, nk + 1)
    h = _rows_h(B, zeros=False)
    cb = [0.6 / (j + 1) * (-1) ** j for j in range(nk)]
    ce = [1e-3 * (j + 1) * (-1) ** (j + 1) for j in range(nk)]
    atol, rtol = 1e-5, 1e-4
    unew = torch.full((B * d,), float("nan"), dtype=dtype, device=DEV)
    enorm = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    _rows_form(dtype, B, d, [unew, u] + K)
    ops.rows_combine_wrms(B, d, unew, u, K, cb, ce, h, atol, rtol, enorm)
    hb = h.view(B, 1)
    un = u.double().view(B, d).clone()
    for c, k in zip(cb, K):
        un = un + (hb * c) * k.double().view(B, d)
    assert _rows_close(unew.view(B, d), un, dtype)
    # the STORED unew, and the stored uhat: err as the kernel's chain forms it, fma((T)(h_r ce_j), K_j, err) -- fp32 products are
    # exact in fp64, one rounding per step -- so for fp32 states only the rounding of tol and of the quotient is left (5e-7)
    un = unew.double().view(B, d)
    err = torch.zeros_like(un)
    for c, k in zip(ce, K):
        err = ((hb * c).to(dtype).double() * k.double().view(B, d) + err).to(dtype).double()
    uh = (un + err).to(dtype).double()
    ref = ((((un - uh) / (atol + rtol * torch.maximum(un.abs(), uh.abs()))) ** 2).sum(1) / d).sqrt()
    assert torch.allclose(enorm, ref, rtol=1e-6 if dtype == torch.float32 else 1e-9, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,d", ROWS_SHAPES)
@pytest.mark.parametrize("nk", range(0, 7))
@pytest.mark.parametrize("with_lam", [True, False])
def test_rows_adj_theta_every_nk(dtype, B, d, nk, with_lam):
    if nk == 0 and not with_lam:
        with pytest.raises(_lib.PnError):                                     # nothing to combine: refused, not launched
            z = torch.zeros(B * d, dtype=dtype, device=DEV)
            HipVecOps(DEV, dtype, B * d).rows_adj_theta(B, d, z, None, 0.0, [], [], _rows_h(B))
        return
    ops = HipVecOps(DEV, dtype, B * d)
    lam, *D = _rows_vecs(B, d, dtype, nk + 1)
    h = _rows_h(B)
    coef = [0.2 * (j + 1) * (-1) ** j for j in range(nk)]
    w = torch.full((B * d,), float("nan"), dtype=dtype, device=DEV)
    _rows_form(dtype, B, d, [w, lam] + D)
    ops.rows_adj_theta(B, d, w, lam if with_lam else None, 0.4, D, coef, h)
    hb = h.view(B, 1)
    ref = (hb * 0.4) * lam.double().view(B, d) if with_lam else torch.zeros(B, d, dtype=torch.float64, device=DEV)
    for c, x in zip(coef, D):
        ref = ref + (hb * c) * x.double().view(B, d)
    assert _rows_close(w.view(B, d), ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,d", ROWS_SHAPES)
@pytest.mark.parametrize("nk", range(0, 8))
def test_rows_adj_accum_every_nk_with_masked_forcing(dtype, B, d, nk):
    ops = HipVecOps(DEV, dtype, B * d)
    T, n = 3, B * d
    lam, *X = _rows_vecs(B, d, dtype, nk + 1)
    gg = _randn((T, n), dtype, 5 + nk)
    hit = (torch.randint(0, T + 1, (B,), generator=torch.Generator().manual_seed(B + d)) - 1).to(torch.int32).to(DEV)
    assert int((hit < 0).sum()) > 0 and int((hit >= 0).sum()) > 0
    out = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
    vec = _rows_form(dtype, B, d, [out, lam, gg] + X)
    assert not vec or gg.stride(0) % _vw(dtype) == 0
    ops.rows_adj_accum(B, d, out, lam, X, gg, gg.stride(0), hit, T)
    ref = lam.double().view(B, d).clone()
    for x in X:
        ref = ref + x.double().view(B, d)
    for i in range(T):
        ref = ref + torch.where((hit == i).view(B, 1), gg[i].double().view(B, d), torch.zeros_like(ref))
    assert _rows_close(out.view(B, d), ref, dtype)
    inplace = lam.clone()
    ops.rows_adj_accum(B, d, inplace, inplace, X, gg, gg.stride(0), hit, T)
    assert torch.equal(inplace, out)


@pytest.mark.parametrize("dtype,d,group", [(torch.float32, 5, 2), (torch.float32, 512, 128), (torch.float32, 4099, 256),
                                           (torch.float64, 5, 4), (torch.float64, 256, 128), (torch.float64, 4099, 256)])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_a_nan_or_inf_row_keeps_to_itself(dtype, d, group, poison):
    """a row's result does not depend on its batch.  One row of a stage derivative is NaN (or inf): that row's norm
    is NaN (inf: not finite -- un - uhat is inf - inf, or inf / inf once the tolerance is infinite too, in any arithmetic), and
    every other row's norm and new state are the bits of the clean run.  The three group sizes: a group inside a wave (shuffles
    of width G), two waves and four waves per row (LDS); the poisoned row shares its workgroup with clean ones when G < 256."""
    assert _group(dtype, d) == group
    B, bad = 300, 5
    assert 256 // group == 1 or bad % (256 // group) != 0                     # not the first row of its workgroup
    ops = HipVecOps(DEV, dtype, B * d)
    u, k1, k2, k3 = _rows_vecs(B, d, dtype, 4)
    h = _rows_h(B, zeros=False)
    cb, ce = [0.6, 0.4, -0.2], [1e-3, -2e-3, 5e-4]

    def run(K):
        unew = torch.full((B * d,), float("nan"), dtype=dtype, device=DEV)
        enorm = torch.full((B,), -1.0, dtype=torch.float64, device=DEV)
        ops.rows_combine_wrms(B, d, unew, u, K, cb, ce, h, 1e-5, 1e-4, enorm)
        return unew.view(B, d), enorm
    clean_u, clean_e = run([k1, k2, k3])
    assert bool(torch.isfinite(clean_e).all()) and bool((clean_e > 0).all())
    k2p = k2.clone()
    k2p.view(B, d)[bad] = poison
    got_u, got_e = run([k1, k2p, k3])
    if math.isnan(poison):
        assert math.isnan(float(got_e[bad]))
    else:
        assert not math.isfinite(float(got_e[bad]))
    keep = torch.arange(B, device=DEV) != bad
    assert torch.equal(got_e[keep], clean_e[keep])
    assert torch.equal(got_u[keep], clean_u[keep])
