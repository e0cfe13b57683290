"""-m gpu: every operand count of every count-dispatching entry point, in both dtypes and both forms of its kernel, against fp64
host arithmetic.  The launchers turn the run-time count into a template argument (pn::with_count, csrc/pn_dispatch.h); a count
that reached the neighbouring instantiation would drop an operand or read one that was never set.

Operand j holds (j + 1) / 8 plus a little noise and every coefficient is positive, so nothing cancels: a dropped or doubled
operand moves the result by at least 0.02, the comparisons below allow 1e-5 at the most.  The bounds are those of the tests that
own each kernel (test_gpu_kernel_variants.py, test_gpu_kernels.py, test_gpu_time_grads.py, test_gpu_sample_adapt.py).

Flat kernels: n = 1027 elements -- in fp32 one workgroup of 256 four-wide vectors and a ragged tail of 3, in fp64 two full
workgroups, a third with one vector, and a tail of 1.  Row kernels: B = 5 rows (no multiple of the rows per workgroup) of d = 18
(fp64: nine 16-byte chunks; fp32: a ragged row, which only the scalar form takes) and of d = 20, where fp32 has a 16-byte form
too.  The scalar form is reached by placing ONE operand -- the last of the pointer table, so that the alignment test has to look
at every entry -- one element past a 16-byte boundary; each test asserts the launcher's predicate on the tensors it passes."""
import math

import numpy as np
import pytest
import torch

from _wrms_cases import stored_uhat, wrms_ref
from conftest import require_gpu
from pnode_amd._vecops import HipVecOps
from test_gpu_kernel_variants import _maxdiff, _rows_close, _tol, _vector_form, _vw

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
FORMS = ["vector", "scalar"]
N = 1027
ROWS = [(5, 18), (5, 20)]


@pytest.fixture(autouse=True)
def _gpu():
    require_gpu()


def _operand(j, n, dtype, off=0):
    """Operand j: (j + 1) / 8 + noise in [0, 0.05), `off` elements past a 16-byte boundary."""
    st = torch.empty(n + 4, dtype=dtype, device=DEV)
    assert st.data_ptr() % 16 == 0
    v = st[off: off + n]
    v.copy_((j + 1) / 8.0 + 0.05 * torch.rand(n, generator=torch.Generator().manual_seed(100 + j), dtype=torch.float64).to(DEV))
    return v


def _table(count, n, dtype, form, first=1):
    """`count` operands first, first + 1, ...; scalar form: the last one is misaligned."""
    return [_operand(first + j, n, dtype, 1 if form == "scalar" and j == count - 1 else 0) for j in range(count)]


def _fixed(j, n, dtype, form, count):
    """An operand outside the pointer table; it carries the misalignment when the table is empty."""
    return _operand(j, n, dtype, 1 if form == "scalar" and count == 0 else 0)


def _coefs(count):
    return [0.2 + 0.1 * j for j in range(count)]


def _d(t):
    return t.double().cpu()


def _close(a, ref, dtype, factor=1):
    return torch.allclose(_d(a), ref, rtol=factor * _tol(dtype), atol=factor * _tol(dtype))


def _nan(n, dtype):
    out = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
    assert out.data_ptr() % 16 == 0
    return out


def test_the_flat_length_has_a_full_workgroup_a_partial_one_and_a_tail():
    assert N // 4 == 256 and N % 4 == 3                    # fp32: exactly one workgroup of vectors, then the tail
    assert N // 2 == 2 * 256 + 1 and N % 2 == 1            # fp64: two full workgroups, one vector in the third, then the tail


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_lincomb_family_every_count(dtype, form):
    """pn_lincomb (1..8), pn_rk_stage (0..7), pn_adj_theta (with lambda 0..7, without 1..8), pn_adj_accum (0..7, with forcing 0..6,
    fused second output): torch.allclose at the tolerance of test_lincomb_family_default_geometry_against_fp64."""
    ops = HipVecOps(DEV, dtype, N)
    vec = form == "vector"
    for nin in range(1, 9):
        xs, cs = _table(nin, N, dtype, form), _coefs(nin)
        out = _nan(N, dtype)
        assert _vector_form(dtype, [out] + xs) == vec
        ops.lincomb(out, xs, cs)
        assert _close(out, sum(c * _d(x) for c, x in zip(cs, xs)), dtype), ("lincomb", nin)
    for nk in range(0, 8):
        u, K, cs = _fixed(0, N, dtype, form, nk), _table(nk, N, dtype, form), _coefs(nk)
        y = _nan(N, dtype)
        assert _vector_form(dtype, [y, u] + K) == vec
        ops.rk_stage(y, u, K, cs)
        assert _close(y, _d(u) + sum(c * _d(k) for c, k in zip(cs, K)), dtype), ("rk_stage", nk)
    for with_lam in (True, False):
        for nk in (range(0, 8) if with_lam else range(1, 9)):
            lam = _fixed(0, N, dtype, form, nk) if with_lam else None
            D, cs = _table(nk, N, dtype, form), _coefs(nk)
            w = _nan(N, dtype)
            assert _vector_form(dtype, [w] + ([lam] if with_lam else []) + D) == vec
            ops.adj_theta(w, lam, 0.75, D, cs)
            ref = sum(c * _d(x) for c, x in zip(cs, D)) + (0.75 * _d(lam) if with_lam else 0.0)
            assert _close(w, ref, dtype), ("adj_theta", with_lam, nk)
    for with_f in (False, True):
        for nk in range(0, 7 if with_f else 8):
            lam, D, cs = _fixed(0, N, dtype, form, nk), _table(nk, N, dtype, form), _coefs(nk)
            f = _operand(9, N, dtype) if with_f else None
            lam_out, w_next = _nan(N, dtype), _nan(N, dtype)
            assert _vector_form(dtype, [lam_out, w_next, lam] + D + ([f] if with_f else [])) == vec
            ops.adj_accum(lam_out, lam, D, cs, f, w_next, 0.5)
            ref = _d(lam) + sum(c * _d(x) for c, x in zip(cs, D)) + (_d(f) if with_f else 0.0)
            assert _close(lam_out, ref, dtype) and _close(w_next, 0.5 * ref, dtype), ("adj_accum", with_f, nk)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_combine_wrms_every_count(dtype, form):
    """pn_rk_combine_wrms, 1..7 stage derivatives, writing unew and not (first same as last): unew and the norm as in
    test_combine_wrms_store_policy_and_vectors_per_thread -- the norm from the STORED unew and the err of the kernel's chain."""
    ops = HipVecOps(DEV, dtype, N)
    npd = np.float32 if dtype == torch.float32 else np.float64
    atol, rtol = 1e-4, 1e-4
    for write in (True, False):
        for nk in range(1, 8):
            u, K = _operand(0, N, dtype), _table(nk, N, dtype, form)
            cb, ce = _coefs(nk), [1e-4 * (j + 1) for j in range(nk)]
            unew = _nan(N, dtype) if write else None
            assert _vector_form(dtype, [u] + K + ([unew] if write else [])) == (form == "vector")
            ops.combine_wrms(unew, u, K, cb, ce, atol, rtol)
            got = ops.read_enorm()
            if write:
                assert _close(unew, _d(u) + sum(c * _d(k) for c, k in zip(cb, K)), dtype, 4), nk
            un = (unew if write else u).cpu().numpy()
            err = np.zeros(N, dtype=npd)
            for c, k in zip(ce, K):
                err = (np.float64(npd(c)) * k.cpu().numpy().astype(np.float64) + err.astype(np.float64)).astype(npd)
            want = wrms_ref(un, stored_uhat(un, err), atol, rtol)
            assert math.isfinite(got) and got == pytest.approx(want, rel=1e-6 if dtype == torch.float32 else 1e-9), (write, nk)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_dots_every_count(dtype, form):
    """pn_dots, 1..8 products in one launch: the bound of test_dots."""
    ops = HipVecOps(DEV, dtype, N)
    for nk in range(1, 9):
        x, ys = _operand(0, N, dtype), _table(nk, N, dtype, form)
        assert _vector_form(dtype, [x] + ys) == (form == "vector")
        got = ops.dots(x, ys)
        scale = float(x.double().norm() * max(y.double().norm() for y in ys))
        assert len(got) == nk
        for j, (g, y) in enumerate(zip(got, ys)):
            assert abs(g - float(torch.dot(_d(x), _d(y)))) <= 1e-12 * scale, (nk, j)


def _matrix(m, n, dtype, first):
    """m rows (operands first, first + 1, ...) with a row stride that is a multiple of the vector width."""
    vw = _vw(dtype)
    ld = -(-n // vw) * vw
    st = torch.full((m, ld), float("nan"), dtype=dtype, device=DEV)
    for o in range(m):
        st[o, :n] = _operand(first + o, n, dtype)
    assert st.data_ptr() % 16 == 0 and st.stride(0) % vw == 0
    return st[:, :n]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_dense_output_every_count(dtype, form):
    """pn_rk_dense_eval (nk 1..7) and pn_rk_dense_adjoint (nd 0..7 with G, 1..7 without): the bounds of
    test_dense_eval_16_byte_form / test_dense_adjoint_16_byte_form."""
    ops = HipVecOps(DEV, dtype, N)
    m = 3
    eps = 1e-5 if dtype == torch.float32 else 1e-13
    for nk in range(1, 8):
        u, K = _operand(0, N, dtype), _table(nk, N, dtype, form)
        coefs = [[0.1 * (o + 1) + 0.05 * j for j in range(nk)] for o in range(m)]
        out = _matrix(m, N, dtype, 20)
        out[:] = float("nan")
        assert _vector_form(dtype, [u, out] + K, out.stride(0)) == (form == "vector")
        ops.dense_eval(out, u, K, coefs)
        cq = torch.tensor(coefs, dtype=torch.float64).to(dtype).double()
        ref = _d(u)[None, :] + cq @ torch.stack([_d(k) for k in K])
        assert _maxdiff(out, ref) <= eps * float(ref.abs().max()), nk
    g = _matrix(m, N, dtype, 10)
    gd = _d(g)
    for with_g in (True, False):
        for nd in range(0 if with_g else 1, 8):
            D = [_nan(N, dtype) for _ in range(nd)]
            G = _nan(N, dtype) if with_g else None
            if form == "scalar":                                # the last output of the table, or G when there is none
                shifted = torch.full((N + 4,), float("nan"), dtype=dtype, device=DEV)[1: 1 + N]
                if nd:
                    D[-1] = shifted
                else:
                    G = shifted
            coefs = [[0.1 * (o + 1) + 0.05 * j for j in range(nd)] for o in range(m)]
            assert _vector_form(dtype, [g] + D + ([G] if with_g else []), g.stride(0)) == (form == "vector")
            ops.dense_adjoint(D, G, g, coefs, accumulate=False)
            tol = eps * math.sqrt(m)
            if nd:
                want = torch.tensor(coefs, dtype=torch.float64).to(dtype).double().t() @ gd
                assert _maxdiff(torch.stack(D), want) <= tol * max(float(want.abs().max()), 1.0), (with_g, nd)
            if with_g:
                want = gd.sum(0)
                assert _maxdiff(G, want) <= tol * max(float(want.abs().max()), 1.0), (with_g, nd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_time_gradient_reductions_every_count(dtype, form):
    """pn_tgrad_dots (np 1..7) and pn_rk_dense_tgrad (nk 1..7): the bound of test_tgrad_vector_form_past_the_grid_cap."""
    ops = HipVecOps(DEV, dtype, N)
    for np_ in range(1, 8):
        xs, ys, cs = _table(np_, N, dtype, "vector"), _table(np_, N, dtype, form, first=3), _coefs(np_)
        assert _vector_form(dtype, xs + ys) == (form == "vector")
        slot = torch.full((3,), 0.5, dtype=torch.float64, device=DEV)
        ops.tgrad_dots(slot[1:2], xs, ys, cs, accumulate=False)
        ref = sum(c * float(_d(x) @ _d(y)) for c, x, y in zip(cs, xs, ys))
        assert abs(float(slot[1]) - ref) <= 1e-12 * max(1.0, abs(ref)) * N ** 0.5, np_
        assert float(slot[0]) == 0.5 and float(slot[2]) == 0.5
    m = 3
    g = _matrix(m, N, dtype, 10)
    for nk in range(1, 8):
        K = _table(nk, N, dtype, form)
        co = torch.tensor([[0.1 * (o + 1) + 0.05 * j for j in range(nk)] for o in range(m)], dtype=torch.float64)
        assert _vector_form(dtype, [g] + K, g.stride(0)) == (form == "vector")
        acc = torch.zeros(m + 2, dtype=torch.float64, device=DEV)
        ops.dense_tgrad(acc[1:m + 1], g, K, co.tolist(), accumulate=False)
        ref = ((_d(g) @ torch.stack([_d(k) for k in K]).t()) * co).sum(1)
        a = acc.cpu()
        assert float((a[1:m + 1] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())) * N ** 0.5, nk
        assert float(a[0]) == 0.0 and float(a[m + 1]) == 0.0


def _rows_vec(dtype, d, tensors):
    return d % _vw(dtype) == 0 and all(t.data_ptr() % 16 == 0 for t in tensors)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,d", ROWS)
def test_rows_kernels_every_count(dtype, form, B, d):
    """pn_rows_stage (1..7), pn_rows_combine_wrms (1..7, writing and not), pn_rows_adj_theta (with lambda 0..6, without 1..6),
    pn_rows_adj_accum (0..7): the bounds of section D of test_gpu_kernel_variants.py."""
    n = B * d
    ops = HipVecOps(DEV, dtype, n)
    ragged = d % _vw(dtype) != 0
    assert ragged == ((d, dtype) == (18, torch.float32))
    vec = form == "vector" and not ragged
    h = (0.05 + 0.1 * torch.arange(1, B + 1, dtype=torch.float64)).to(DEV)
    hb = h.view(B, 1).cpu()
    rows = lambda t: _d(t).view(B, d)   # noqa: E731
    for nk in range(1, 8):
        u, K, cs = _operand(0, n, dtype), _table(nk, n, dtype, form), _coefs(nk)
        y = _nan(n, dtype)
        assert _rows_vec(dtype, d, [y, u] + K) == vec
        ops.rows_stage(B, d, y, u, K, cs, h)
        ref = rows(u) + sum((hb * c) * rows(k) for c, k in zip(cs, K))
        assert _rows_close(y.view(B, d).cpu(), ref, dtype), ("stage", nk)
    atol, rtol = 1e-5, 1e-4
    for write in (True, False):
        for nk in range(1, 8):
            u, K = _operand(0, n, dtype), _table(nk, n, dtype, form)
            cb, ce = _coefs(nk), [1e-3 * (j + 1) for j in range(nk)]
            unew = _nan(n, dtype) if write else None
            enorm = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
            assert _rows_vec(dtype, d, [u] + K + ([unew] if write else [])) == vec
            ops.rows_combine_wrms(B, d, unew, u, K, cb, ce, h, atol, rtol, enorm)
            if write:
                assert _rows_close(unew.view(B, d).cpu(), rows(u) + sum((hb * c) * rows(k) for c, k in zip(cb, K)), dtype), nk
            un = rows(unew if write else u)
            err = torch.zeros_like(un)
            for c, k in zip(ce, K):
                err = ((hb * c).to(dtype).double() * rows(k) + err).to(dtype).double()
            uh = (un + err).to(dtype).double()
            ref = ((((un - uh) / (atol + rtol * torch.maximum(un.abs(), uh.abs()))) ** 2).sum(1) / d).sqrt()
            assert torch.allclose(enorm.cpu(), ref, rtol=1e-6 if dtype == torch.float32 else 1e-9, atol=1e-12), (write, nk)
    for with_lam in (True, False):
        for nk in range(0 if with_lam else 1, 7):
            lam = _fixed(0, n, dtype, form, nk) if with_lam else None
            D, cs = _table(nk, n, dtype, form), _coefs(nk)
            w = _nan(n, dtype)
            assert _rows_vec(dtype, d, [w] + ([lam] if with_lam else []) + D) == vec
            ops.rows_adj_theta(B, d, w, lam, 0.4, D, cs, h)
            ref = sum((hb * c) * rows(x) for c, x in zip(cs, D)) + ((hb * 0.4) * rows(lam) if with_lam else 0.0)
            assert _rows_close(w.view(B, d).cpu(), ref, dtype), ("adj_theta", with_lam, nk)
    for nk in range(0, 8):
        lam, X = _fixed(0, n, dtype, form, nk), _table(nk, n, dtype, form)
        out = _nan(n, dtype)
        assert _rows_vec(dtype, d, [out, lam] + X) == vec
        ops.rows_adj_accum(B, d, out, lam, X, None, 0, None, 0)
        assert _rows_close(out.view(B, d).cpu(), rows(lam) + sum(rows(x) for x in X), dtype), ("adj_accum", nk)
    torch.cuda.synchronize()
