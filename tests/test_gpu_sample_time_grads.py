"""-m gpu: the kernels behind dL/dt of a -pn_adapt_scope sample solve (pn_rows_tgrad_dots, pn_rows_dense_tgrad, pn_rows_tgrad_scatter,
pn_rows_tgrad_reduce; csrc/pn_rows.hip) against fp64 host sums, and whole solves on the device.

Shapes: the smallest that reach each path of the row geometry -- d = 2 (one thread per row, many rows per wave), d = 3 fp32 (a
ragged row: the scalar form), d = 8 fp32 (two chunks, the vector form), d = 130 fp64 (65 chunks, a group of 128: two waves through
LDS), d = 1025 fp32 (257 chunks, a group of 256 that strides, ragged tail); bases offset by one element (unaligned); B = 1, 5 and
one row more than a workgroup holds.

Tolerances.  The kernels and the references both add exact-to-rounding products in double: a sum of m terms carries at most
m * 2^-53 * sum|terms| in either, so the two differ by at most twice that; the bound used is 2 (m + 8) 2^-53 sum|terms| with the
terms taken in absolute value (the 8: the coefficient products and the tree's few extra additions)."""
import ctypes

import pytest
import torch
import torch.nn as nn

from conftest import require_gpu
from pnode_amd import _lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
CASES = [(torch.float32, 2), (torch.float64, 2), (torch.float32, 3), (torch.float32, 8), (torch.float64, 130), (torch.float32, 1025)]
T = 40


def _ops(dtype, n):
    from pnode_amd.petsc_adjoint import HipVecOps
    return HipVecOps(require_gpu(), dtype, n)


def _geom(dtype, d):
    vw = 4 if dtype == torch.float32 else 2
    nch = (d + vw - 1) // vw
    G = 1
    while G < nch and G < 256:
        G *= 2
    return vw, G


def _shapes():
    return [(dt, d, B) for dt, d in CASES for B in (1, 5, 256 // _geom(dt, d)[1] + 1)]


def _vecs(B, d, dtype, k, dev, offset, seed=0):
    g = torch.Generator().manual_seed(B * 131 + d * 7 + k + seed)
    return [(2.0 * torch.rand(B * d + offset, generator=g, dtype=torch.float64) - 1.0).to(dtype).to(dev)[offset:] for _ in range(k)]


@pytest.mark.parametrize("dtype,d,B", _shapes())
@pytest.mark.parametrize("offset", [0, 1])
def test_rows_tgrad_dots(dtype, d, B, offset):
    ops = _ops(dtype, B * d)
    dev = ops.device
    coefs = [0.75, -1.5, 2.0]
    xs = _vecs(B, d, dtype, 3, dev, offset)
    ys = _vecs(B, d, dtype, 3, dev, offset, seed=5)

    def run(o, B_, xs_, ys_):
        acc = torch.full((B_,), float("nan"), dtype=torch.float64, device=dev)
        o.rows_tgrad_dots(B_, d, acc, xs_, ys_, coefs, accumulate=False)
        first = acc.clone()
        o.rows_tgrad_dots(B_, d, acc, xs_[:1], ys_[:1], [0.5], accumulate=True)
        return first.cpu(), acc.cpu()

    first, second = run(ops, B, xs, ys)
    X = [x.double().cpu().view(B, d) for x in xs]
    Y = [y.double().cpu().view(B, d) for y in ys]
    ref = sum(c * (x * y).sum(1) for c, x, y in zip(coefs, X, Y))
    mag = sum(abs(c) * (x * y).abs().sum(1) for c, x, y in zip(coefs, X, Y))
    bound = 2 * (3 * d + 8) * EPS * mag
    print("pn_rows_tgrad_dots %s d=%d B=%d offset=%d: worst error / bound %.3f" % (dtype, d, B, offset, float(((first - ref).abs() / bound).max())))
    assert bool(((first - ref).abs() <= bound).all())
    ref2 = ref + 0.5 * (X[0] * Y[0]).sum(1)
    assert bool(((second - ref2).abs() <= bound + 2 * (d + 8) * EPS * 0.5 * (X[0] * Y[0]).abs().sum(1)).all())
    # the same bits again, for a row alone (its batch does not matter) and, where the vector form exists, in both forms
    assert torch.equal(run(ops, B, xs, ys)[0], first)
    for r in sorted({0, B - 1}):
        one = run(_ops(dtype, d), 1, [x.view(B, d)[r].clone() for x in xs], [y.view(B, d)[r].clone() for y in ys])[0]
        assert torch.equal(one, first[r:r + 1]), r
    if offset and d % _geom(dtype, d)[0] == 0:
        assert torch.equal(run(ops, B, [x.clone() for x in xs], [y.clone() for y in ys])[0], first)


def _table():
    _, P = _lib.get_tableau_dense("5dp")
    cols = [j for j in range(_lib.PN_MAX_STAGES) if any(v != 0.0 for v in P[j])]
    pv = [v for j in cols for v in list(P[j]) + [0.0] * (_lib.PN_DENSE_MAX_POW - len(P[j]))]
    return len(cols), (ctypes.c_double * len(pv))(*pv)


def _draw(B, shift=0):
    """A round's log for B rows, the kinds in turn: 0 an empty range, 1 h_eff = 0 with a stale range (nothing may be written), 2 a
    range of 36 outputs (more than 32, five tiles), 3 two outputs."""
    times = torch.linspace(0.0, 0.25, T, dtype=torch.float64)
    dt = 0.25 / (T - 1)
    r = torch.arange(B)
    cat = (r + shift) % 4
    i0 = 1 + (r * 7) % 30
    log_d = torch.zeros(3, B, dtype=torch.float64)
    rng = torch.zeros(2, B, dtype=torch.int32)
    t_r = times[i0] - 0.3 * dt
    h = torch.full((B,), 2.5 * dt, dtype=torch.float64)
    lo, hi = i0.clone(), i0 + 2
    hi = torch.where(cat == 0, lo, hi)
    h = torch.where(cat == 1, torch.zeros_like(h), h)
    lo = torch.where(cat == 2, torch.ones_like(lo), lo)
    hi = torch.where(cat == 2, torch.full_like(hi, 37), hi)
    t_r = torch.where(cat == 2, torch.full_like(t_r, 0.4 * dt), t_r)
    h = torch.where(cat == 2, torch.full_like(h, 36.5 * dt), h)
    log_d[0], log_d[1], log_d[2] = h, t_r, t_r
    rng[0], rng[1] = lo.to(torch.int32), hi.to(torch.int32)
    return times, cat, log_d, rng


@pytest.mark.parametrize("dtype,d,B", _shapes())
@pytest.mark.parametrize("offset", [0, 1])
def test_rows_dense_tgrad(dtype, d, B, offset):
    ops = _ops(dtype, B * d)
    dev = ops.device
    n = B * d
    nk, P = _table()
    Ks = _vecs(B, d, dtype, nk, dev, offset)
    times, cat, log_d, rng = _draw(B, shift=d % 4)
    gen = torch.Generator().manual_seed(B + 3 * d)
    g = (2.0 * torch.rand(offset + T * n, generator=gen, dtype=torch.float64) - 1.0).to(dtype).to(dev)[offset:].view(T, n)
    theta = torch.zeros(T, B, dtype=torch.float64)
    dcoef = torch.zeros(T, B, nk, dtype=torch.float64)
    _lib.check(_lib.load().pn_rows_dense_tgrad_host(B, T, times.data_ptr(), log_d.data_ptr(), rng.data_ptr(), nk, P, theta.data_ptr(),
                                                    dcoef.data_ptr()))

    def run(o, B_, g_, Ks_, log_d_, rng_):
        erow = torch.full((T, B_), float("nan"), dtype=torch.float64, device=dev)
        o.rows_dense_tgrad(B_, d, erow, g_, Ks_, times.to(dev), P, rng_.to(dev), log_d_.to(dev))
        return erow.cpu()

    erow = run(ops, B, g, Ks, log_d, rng)
    served = torch.zeros(T, B, dtype=torch.bool)
    for r in range(B):
        if float(log_d[0, r]) > 0.0:
            served[int(rng[0, r]):int(rng[1, r]), r] = True
    assert torch.equal(~torch.isnan(erow), served)                 # nothing outside a row's range, nothing for h_eff = 0
    assert B < 4 or (int((rng[1] - rng[0]).max()) > 32 and bool((cat == 1).any()) and bool((cat == 0).any()))
    g64 = g.double().cpu().view(T, B, d)
    K64 = torch.stack([k.double().cpu().view(B, d) for k in Ks])                 # [nk][B][d]
    prod = torch.einsum("obd,jbd->objd", g64, K64)                               # [T][B][nk][d]
    ref = (dcoef * prod.sum(3)).sum(2)
    mag = (dcoef.abs() * prod.abs().sum(3)).sum(2)
    bound = 2 * (nk * d + 8) * EPS * mag
    err = (erow - ref).abs()[served]
    if served.any():
        print("pn_rows_dense_tgrad %s d=%d B=%d offset=%d: worst error / bound %.3f" % (dtype, d, B, offset, float((err / bound[served]).max())))
        assert bool((err <= bound[served]).all())
    assert torch.equal(run(ops, B, g, Ks, log_d, rng).nan_to_num(nan=0.0), erow.nan_to_num(nan=0.0))
    for r in sorted({0, B // 2, B - 1}):
        one = run(_ops(dtype, d), 1, g.view(T, B, d)[:, r].clone(), [k.view(B, d)[r].clone() for k in Ks], log_d[:, r:r + 1].contiguous(),
                  rng[:, r:r + 1].contiguous())
        assert torch.equal(one[:, 0].nan_to_num(nan=0.0), erow[:, r].nan_to_num(nan=0.0)), r
    if offset and d % _geom(dtype, d)[0] == 0:
        al = run(ops, B, g.clone(), [k.clone() for k in Ks], log_d, rng)
        assert torch.equal(al.nan_to_num(nan=0.0), erow.nan_to_num(nan=0.0))


@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("fsal", [False, True])
def test_rows_tgrad_scatter_is_the_host_text(B, dense, fsal):
    """Three reversed rounds and the flush on the device and on host arrays: the same function, the same bits."""
    ops = _ops(torch.float64, B)
    dev = ops.device
    lib = _lib.load()
    nout = T if dense else 4
    gen = torch.Generator().manual_seed(B + 2 * dense + fsal)
    rnd = lambda *s: 2.0 * torch.rand(*s, generator=gen, dtype=torch.float64) - 1.0
    times, _, _, _ = _draw(B)
    if not dense:
        times = times[:nout].clone()
    state = dict(dtrow=rnd(nout, B), held=torch.zeros(B, dtype=torch.float64), iv=torch.full((B,), nout - 1, dtype=torch.int32))
    dstate = {k: v.to(dev) for k, v in state.items()}
    coefs = [0.2, 0.75]
    for k in range(3):
        _, cat, log_d, rng = _draw(B, shift=k)
        hit = torch.where((torch.arange(B) + k) % 3 == 0, nout - 1 - k, -1).to(torch.int32)
        if k == 1:
            hit[B // 2] = nout + 3                     # an index past the outputs counts as none
        rowacc, tb0, tb1, tb2, erow = rnd(B), rnd(B), rnd(B), rnd(B), rnd(nout, B)
        tbars = [tb1, tb2][: 2 - (k == 2)]
        t0 = tb0 if (fsal and k != 1) else None
        opt = lambda x: None if x is None else x.data_ptr()
        _lib.check(lib.pn_rows_tgrad_scatter_host(
            B, nout, state["dtrow"].data_ptr(), rowacc.data_ptr(), len(tbars), (ctypes.c_void_p * 2)(*[x.data_ptr() for x in tbars]),
            (ctypes.c_double * 2)(*coefs), opt(t0), 0.875, int(fsal), log_d.data_ptr(), hit.data_ptr(), rng.data_ptr() if dense else None,
            erow.data_ptr() if dense else None, times.data_ptr() if dense else None, state["held"].data_ptr(), state["iv"].data_ptr(), 0))
        dv = lambda x: None if x is None else x.to(dev)
        ops.rows_tgrad_scatter(B, dstate["dtrow"], dv(rowacc), [dv(x) for x in tbars], coefs[:len(tbars)], dv(t0), 0.875, fsal, dv(log_d),
                               dv(hit), dv(rng) if dense else None, dv(erow) if dense else None, dv(times) if dense else None,
                               dstate["held"], dstate["iv"])
        for key in state:
            assert torch.equal(dstate[key].cpu(), state[key]), (k, key)
        touched = (log_d[0] > 0.0)
        assert B < 4 or (bool(touched.any()) and not bool(touched.all()))
    _lib.check(lib.pn_rows_tgrad_scatter_host(B, nout, state["dtrow"].data_ptr(), None, 0, None, None, None, 0.0, int(fsal), None, None, None,
                                              None, None, state["held"].data_ptr(), state["iv"].data_ptr(), 1))
    ops.rows_tgrad_scatter(B, dstate["dtrow"], None, [], [], None, 0.0, fsal, None, None, None, None, None, dstate["held"], dstate["iv"],
                           flush=True)
    for key in state:
        assert torch.equal(dstate[key].cpu(), state[key]), key
    assert not bool(state["held"].any())


@pytest.mark.parametrize("B", [1, 5, 4097])
def test_rows_tgrad_reduce(B):
    ops = _ops(torch.float64, B)
    dev = ops.device
    nout = 3
    gen = torch.Generator().manual_seed(B)
    dtrow = (2.0 * torch.rand(nout, B, generator=gen, dtype=torch.float64) - 1.0) * torch.logspace(-3, 3, B, dtype=torch.float64)
    d_dev = dtrow.to(dev)
    out = []
    for _ in range(2):
        dt = torch.full((nout,), float("nan"), dtype=torch.float64, device=dev)
        ops.rows_tgrad_reduce(B, d_dev, dt)
        out.append(dt.cpu())
    assert torch.equal(out[0], out[1])
    ref = torch.tensor([sum(row) for row in dtrow.tolist()], dtype=torch.float64)         # in index order, in double
    bound = 2 * max(B - 1, 1) * EPS * dtrow.abs().sum(1)
    assert bool(((out[0] - ref).abs() <= bound).all()), (out[0], ref)
    if B == 1:
        assert torch.equal(out[0], dtrow[:, 0])


# ---------------------------------------------------------------------------------------------------- whole solves
class TimeSpiral(nn.Module):
    """The cubic spiral times 1 + 0.5 sin(5 t), plus a drift in t (tests/test_sample_time_grads.py)."""

    def __init__(self, dtype):
        super().__init__()
        from problems import SpiralTruth
        self.inner = SpiralTruth(dtype)
        self.v = nn.Parameter(torch.tensor([0.3, -0.2], dtype=dtype))

    def forward(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        return self.inner(t, y) * (1.0 + 0.5 * torch.sin(5.0 * t)) + self.v * torch.cos(3.0 * t)


def _spread(Bn, dtype=torch.float64):
    g = torch.Generator().manual_seed(0)
    r = torch.logspace(-1.3, 0.3, Bn, dtype=torch.float64)
    ang = 6.28 * torch.rand(Bn, generator=g, dtype=torch.float64)
    return torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=1).to(dtype)


def _solve(y0, dev, mode, scope="sample", tol=1e-8, times=(0.0, 0.05, 0.12, 0.2)):
    from pnode_amd import options, petsc_adjoint
    options.clear()
    options.set_option("ts_rk_type", "5dp")
    options.set_option("ts_rtol", tol)
    options.set_option("ts_atol", tol)
    options.set_option("pn_adapt_scope", scope)
    options.set_option("pn_output_times", mode)
    try:
        f = TimeSpiral(y0.dtype).to(dev)
        ode = petsc_adjoint.ODEPetsc()
        y = y0.to(dev).clone().requires_grad_(True)
        ode.setupTS(y, f, step_size=0.2, method="dopri5")
        t = torch.tensor(times, dtype=torch.float64, device=dev, requires_grad=True)
        pred = ode.odeint_adjoint(y, t)
        w0 = (1.0 + 0.3 * torch.sin(7.0 * y0.double())).to(pred.dtype).to(dev)
        w = torch.stack([w0 * (1.0 + 0.1 * i) for i in range(pred.shape[0])])
        (pred * w).sum().backward()
        return t.grad.cpu(), (None if scope == "batch" else ode.sample_time_grads.cpu()), ode
    finally:
        options.clear()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())


@pytest.mark.parametrize("mode", ["match", "interpolate"])
def test_fp64_columns_are_the_batch_of_one_solves_on_the_device(mode):
    dev = require_gpu()
    y0 = _spread(6)
    gt, dtrow, ode = _solve(y0, dev, mode)
    assert gt.shape == (4,) and dtrow.shape == (4, 6) and dtrow.dtype == torch.float64
    assert int(ode.sample_rejections.max()) > 0 and int(ode.sample_steps.max()) >= 2 * int(ode.sample_steps.min())
    worst = 0.0
    for r in range(6):
        one, _, oode = _solve(y0[r:r + 1], dev, mode, scope="batch")
        assert int(ode.sample_steps[r]) == oode.num_steps
        worst = max(worst, _rel(dtrow[:, r], one))
    print("dL/dt on the device, %s: columns against batch-of-one %.2e" % (mode, worst))
    assert worst <= 1e-11
    bound = 5 * EPS * dtrow.abs().sum(1)
    assert bool(((gt - dtrow.sum(1)).abs() <= bound).all())
    gt2, dtrow2, _ = _solve(y0, dev, mode)
    assert torch.equal(gt, gt2) and torch.equal(dtrow, dtrow2)
    _, half, _ = _solve(y0[3:], dev, mode)
    assert torch.equal(dtrow[:, 3:], half)


@pytest.mark.parametrize("mode", ["match", "interpolate"])
def test_fp32_against_the_fp64_engine(mode):
    """The project's bar for fp32 gradients (tests/test_gpu_configs.py): within 1e-5 relative of the fp64 engine run with the same
    options."""
    dev = require_gpu()
    y0 = _spread(6)
    g32, d32, o32 = _solve(y0.float(), dev, mode, tol=1e-4)
    g64, d64, o64 = _solve(y0.float().double(), dev, mode, tol=1e-4)
    print("dL/dt fp32 against fp64, %s: steps %s / %s, t.grad %.2e, columns %.2e"
          % (mode, o32.sample_steps.tolist(), o64.sample_steps.tolist(), _rel(g32, g64), _rel(d32, d64)))
    assert g32.dtype == torch.float64 and d32.dtype == torch.float64
    assert _rel(g32, g64) <= 1e-5 and _rel(d32, d64) <= 1e-5
