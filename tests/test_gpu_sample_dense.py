"""-m gpu: the row-dense kernels (pn_rows_dense_eval, pn_rows_dense_adjoint, pn_rows_adj_theta_dense; csrc/pn_rows.hip) against
fp64 arithmetic, their plan against the host form of the same text (pn_rows_dense_plan_host), and -pn_adapt_scope sample with
-pn_output_times interpolate end to end on the device against the CPU stand-in (tests/_cpu_rows_dense_ops.py).

Tolerances are those of tests/test_gpu_sample_adapt.py (2e-6 for fp32 states, 1e-14 for fp64, absolute + relative).  The operands
are drawn so that the worst case stays inside them: 40 output times on [0, 0.25], so |c_j| = h |beta_j| <= 0.25, and
  * an output is u + 6 fma terms with |u|, |K_j| <= 1: partial sums below 4, seven roundings of at most half an ulp of that
    (fp32: 7 * 1.2e-7 = 8.4e-7) plus the rounding of the coefficients to the storage type (6 * 0.25 * 6e-8 = 1e-7);
  * D_j and G sum at most 38 cotangent rows with |g| <= 1 / 40: partial sums below 1, 38 roundings of at most 3e-8 = 1.2e-6
    (fp32; fp64: 38 * 5.6e-17)."""
import ctypes

import pytest
import torch

from conftest import require_gpu
from pnode_amd import _lib

pytestmark = pytest.mark.gpu

DS = [1, 2, 5, 512, 4099]
BS = [1, 3, 4096]
FITS = 2 ** 22            # B * d elements per vector of a kernel test (the solution matrix is 40 such rows)
STRIDE = (9000, 512)      # more row groups than the capped grid has workgroups: a second trip of the block-stride loop
T = 40                    # output times: a row of the "many" kind serves 36 > PN_DENSE_CHUNK of them in one launch
NCAT = 6


def _ops(dtype, n):
    from pnode_amd.petsc_adjoint import HipVecOps
    return HipVecOps(require_gpu(), dtype, n)


def _tol(dtype):
    return 2e-6 if dtype == torch.float32 else 1e-14


def _close(a, b, dtype):
    return torch.allclose(a.double(), b, rtol=_tol(dtype), atol=_tol(dtype))


def _shapes():
    return [(B, d) for d in DS for B in BS if B * d <= FITS] + [STRIDE]


def _vecs(B, d, dtype, k, dev, offset=0, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(B * 131 + d * 7 + k + seed)
    return [((2.0 * torch.rand(B * d + offset, generator=g, dtype=torch.float64) - 1.0) * scale).to(dtype).to(dev)[offset:] for _ in range(k)]


def _table():
    """(the used columns of 5dp's extension, their rows of the polynomial table as the entry points take them)"""
    _, P = _lib.get_tableau_dense("5dp")
    cols = [j for j in range(_lib.PN_MAX_STAGES) if any(v != 0.0 for v in P[j])]
    pv = [v for j in cols for v in list(P[j]) + [0.0] * (_lib.PN_DENSE_MAX_POW - len(P[j]))]
    return cols, (ctypes.c_double * len(pv))(*pv)


def _draw(B, shift):
    """One round's log for B rows, the kinds in turn: 0 an empty range, 1 one output, 2 more than PN_DENSE_CHUNK outputs, 3 h = 0
    (rejected or finished), 4 a landing exactly on an output (after two interpolated ones), 5 the final step (one output inside)."""
    times = torch.linspace(0.0, 0.25, T, dtype=torch.float64)
    dt = 0.25 / (T - 1)
    r = torch.arange(B)
    cat = (r + shift) % NCAT
    i0 = 1 + (r * 7) % 30
    ti = times[i0]
    t_r = ti + 0.2 * dt
    tnew = ti + 0.7 * dt
    nxt = i0 + 1
    tnew = torch.where(cat == 1, times[i0 + 1] + 0.5 * dt, tnew)
    t_r = torch.where(cat == 2, torch.full_like(t_r, 0.3 * dt), t_r)
    tnew = torch.where(cat == 2, times[36] + 0.5 * dt, tnew)
    nxt = torch.where(cat == 2, torch.ones_like(nxt), nxt)
    tnew = torch.where(cat == 4, times[i0 + 3], tnew)
    t_r = torch.where(cat == 5, times[T - 3] + 0.4 * dt, t_r)
    tnew = torch.where(cat == 5, times[T - 1], tnew)
    nxt = torch.where(cat == 5, torch.full_like(nxt, T - 2), nxt)
    heff = torch.where(cat == 3, torch.zeros_like(t_r), tnew - t_r)
    tnew = torch.where(cat == 3, t_r, tnew)
    log_d = torch.zeros(3, B, dtype=torch.float64)
    log_d[0], log_d[1], log_d[2] = heff, t_r, t_r
    hit = torch.where(cat == 5, 1, -1).to(torch.int32)
    return times, cat, log_d, tnew.contiguous(), hit, nxt.to(torch.int32)


def _host_plan(B, times, log_d, tnew, hit, nxt, nk, P):
    lib = _lib.load()
    hit, nxt = hit.clone(), nxt.clone()
    rng = torch.full((2, B), -7, dtype=torch.int32)
    coef = torch.zeros(T, B, nk, dtype=torch.float64)
    _lib.check(lib.pn_rows_dense_plan_host(B, T, times.data_ptr(), log_d.data_ptr(), tnew.data_ptr(), hit.data_ptr(), nxt.data_ptr(),
                                           rng.data_ptr(), nk, P, coef.data_ptr()))
    return rng, hit, nxt, coef


def _expected_kinds(B, cat, rng, hit):
    n = rng[1] - rng[0]
    for c, want_n, want_hit in ((0, 0, False), (1, 1, False), (2, 36, False), (3, 0, False), (4, 2, True), (5, 1, True)):
        m = cat == c
        if m.any():
            assert (n[m] == want_n).all() and ((hit[m] >= 0) == want_hit).all(), c
    assert int(n.max()) > _lib.PN_DENSE_CHUNK or B < NCAT
    assert B < NCAT or all((cat == c).any() for c in range(NCAT))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,d", _shapes())
@pytest.mark.parametrize("offset", [0, 1])
def test_rows_dense_eval(dtype, B, d, offset):
    ops = _ops(dtype, B * d)
    dev = ops.device
    n = B * d
    cols, P = _table()
    nk = len(cols)
    u, unew, *Ks = _vecs(B, d, dtype, 2 + nk, dev, offset)
    times, cat, log_d, tnew, hit0, nxt0 = _draw(B, shift=d % NCAT)
    rng_h, hit_h, nxt_h, coef = _host_plan(B, times, log_d, tnew, hit0, nxt0, nk, P)
    _expected_kinds(B, cat, rng_h, hit_h)

    def run(B_, u_, unew_, Ks_, log_d_, tnew_, hit_, nxt_, off):
        o = _ops(dtype, B_ * d)
        sol = torch.full((off + T * B_ * d,), float("nan"), dtype=dtype, device=dev)[off:].view(T, B_ * d)
        hit_d, nxt_d = hit_.to(dev), nxt_.to(dev)
        rng_d = torch.full((2, B_), -7, dtype=torch.int32, device=dev)
        o.rows_dense_eval(B_, d, sol, times.to(dev), u_, Ks_, P, unew_, log_d_.to(dev), tnew_.to(dev), hit_d, nxt_d, rng_d)
        return sol, rng_d.cpu(), hit_d.cpu(), nxt_d.cpu()

    sol, rng_d, hit_d, nxt_d = run(B, u, unew, Ks, log_d, tnew, hit0, nxt0, offset)
    # the device plan is the host function's, exactly
    assert torch.equal(rng_d, rng_h) and torch.equal(hit_d, hit_h) and torch.equal(nxt_d, nxt_h)
    # values: fp64 arithmetic with the host function's coefficients; NaN where no output is served
    ref = torch.full((T, B, d), float("nan"), dtype=torch.float64, device=dev)
    u64, k64 = u.double().view(B, d), [k.double().view(B, d) for k in Ks]
    lo, hi, cf = rng_h[0].to(dev), rng_h[1].to(dev), coef.to(dev)
    for o in range(1, T - 1):
        m = (lo <= o) & (o < hi)
        if m.any():
            acc = u64[m].clone()
            for j in range(nk):
                acc = acc + cf[o, m, j].view(-1, 1) * k64[j][m]
            ref[o, m] = acc
    rows = (hit_h >= 0).nonzero().view(-1)
    copies = torch.zeros(T, B, dtype=torch.bool)
    copies[hit_h[rows].long(), rows] = True
    copies = copies.to(dev)
    ref[copies] = unew.double().view(B, d).expand(T, B, d)[copies]
    got = sol.view(T, B, d)
    served = ~torch.isnan(ref)
    assert torch.equal(torch.isnan(got), ~served)                            # what no row serves is untouched
    assert _close(got[served], ref[served], dtype)
    assert torch.equal(got[copies], unew.view(B, d).expand(T, B, d)[copies])  # copies are copies
    # run to run, and (scalar form) the same bits as the vector form on aligned copies
    again = run(B, u, unew, Ks, log_d, tnew, hit0, nxt0, offset)[0]
    assert torch.equal(again.nan_to_num(nan=0.0), sol.nan_to_num(nan=0.0))
    if offset:
        al = run(B, u.clone(), unew.clone(), [k.clone() for k in Ks], log_d, tnew, hit0, nxt0, 0)[0]
        assert torch.equal(al.nan_to_num(nan=0.0), sol.nan_to_num(nan=0.0))
    # a row's bits do not depend on the batch: rows alone, as batches of one
    for r in sorted({0, B // 2, B - 1}):
        one = run(1, u.view(B, d)[r].clone(), unew.view(B, d)[r].clone(), [k.view(B, d)[r].clone() for k in Ks],
                  log_d[:, r:r + 1].contiguous(), tnew[r:r + 1].clone(), hit0[r:r + 1].clone(), nxt0[r:r + 1].clone(), 0)[0]
        assert torch.equal(one.view(T, d).nan_to_num(nan=0.0), got[:, r].nan_to_num(nan=0.0)), r


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,d", _shapes())
@pytest.mark.parametrize("offset", [0, 1])
def test_rows_dense_adjoint(dtype, B, d, offset):
    ops = _ops(dtype, B * d)
    dev = ops.device
    n = B * d
    cols, P = _table()
    nd = len(cols)
    times, cat, log_d, tnew, hit0, nxt0 = _draw(B, shift=(d + 2) % NCAT)
    rng_h, hit_h, _, coef = _host_plan(B, times, log_d, tnew, hit0, nxt0, nd, P)
    _expected_kinds(B, cat, rng_h, hit_h)
    gen = torch.Generator().manual_seed(B + 3 * d)
    g = ((2.0 * torch.rand(offset + T * n, generator=gen, dtype=torch.float64) - 1.0) / T).to(dtype).to(dev)[offset:].view(T, n)

    def run(off, g_):
        Ds = [torch.full((n + off,), float("nan"), dtype=dtype, device=dev)[off:] for _ in range(nd)]
        G = torch.full((n + off,), float("nan"), dtype=dtype, device=dev)[off:]
        ops.rows_dense_adjoint(B, d, Ds, G, g_, times.to(dev), P, rng_h.to(dev), log_d.to(dev))
        return Ds, G

    Ds, G = run(offset, g)
    g64 = g.double().view(T, B, d)
    lo, hi, cf = rng_h[0].to(dev), rng_h[1].to(dev), coef.to(dev)
    refD = torch.zeros(nd, B, d, dtype=torch.float64, device=dev)
    refG = torch.zeros(B, d, dtype=torch.float64, device=dev)
    for o in range(1, T - 1):
        m = ((lo <= o) & (o < hi)).view(B, 1).double()
        refG = refG + m * g64[o]
        for j in range(nd):
            refD[j] = refD[j] + (m * cf[o, :, j].view(B, 1)) * g64[o]
    assert _close(G.view(B, d), refG, dtype)
    for j in range(nd):
        assert _close(Ds[j].view(B, d), refD[j], dtype), j
    empty = (rng_h[1] == rng_h[0]).to(dev)
    if empty.any():                                     # rows that served nothing get exact zeros
        assert float(G.view(B, d)[empty].abs().max()) == 0.0 and all(float(x.view(B, d)[empty].abs().max()) == 0.0 for x in Ds)
    Ds2, G2 = run(offset, g)
    assert torch.equal(G, G2) and all(torch.equal(a, b) for a, b in zip(Ds, Ds2))
    if offset:
        Ds3, G3 = run(0, g.contiguous().clone())
        assert torch.equal(G, G3) and all(torch.equal(a, b) for a, b in zip(Ds, Ds3))
    # a row alone gives the row's bits
    for r in sorted({0, B // 2, B - 1}):
        one = _ops(dtype, d)
        D1 = [torch.empty(d, dtype=dtype, device=dev) for _ in range(nd)]
        G1 = torch.empty(d, dtype=dtype, device=dev)
        one.rows_dense_adjoint(1, d, D1, G1, g.view(T, B, d)[:, r].contiguous(), times.to(dev), P, rng_h[:, r:r + 1].contiguous().to(dev),
                               log_d[:, r:r + 1].contiguous().to(dev))
        assert torch.equal(G1, G.view(B, d)[r]) and all(torch.equal(a, b.view(B, d)[r]) for a, b in zip(D1, Ds)), r


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,d", _shapes())
@pytest.mark.parametrize("offset", [0, 1])
def test_rows_adj_theta_with_the_unscaled_last_term(dtype, B, d, offset):
    ops = _ops(dtype, B * d)
    dev = ops.device
    lam, x1, x2, D = _vecs(B, d, dtype, 4, dev, offset)
    g = torch.Generator().manual_seed(1 + B)
    h = 0.05 + 0.2 * torch.rand(B, generator=g, dtype=torch.float64)
    if B > 1:
        h[::3] = 0.0
    h = h.to(dev)
    hb = h.view(B, 1)
    w = torch.full((B * d + offset,), float("nan"), dtype=dtype, device=dev)[offset:]
    ops.rows_adj_theta(B, d, w, lam, 0.4, [x1, x2], [0.3, -0.7], h, dense_w=D)
    ref = (hb * 0.4) * lam.double().view(B, d) + (hb * 0.3) * x1.double().view(B, d) + (hb * -0.7) * x2.double().view(B, d) \
        + D.double().view(B, d)
    assert _close(w.view(B, d), ref, dtype)
    # the scaled part is pn_rows_adj_theta's bits; the last term is one addition in the storage type
    w0 = torch.empty_like(w)
    ops.rows_adj_theta(B, d, w0, lam, 0.4, [x1, x2], [0.3, -0.7], h)
    assert torch.equal(w, w0 + D)
    if B > 1:
        assert torch.equal(w.view(B, d)[0], D.view(B, d)[0])                  # h = 0: the cotangent is D alone
    ops.rows_adj_theta(B, d, w, None, 0.0, [x1], [0.3], h, dense_w=D)
    ops.rows_adj_theta(B, d, w0, None, 0.0, [x1], [0.3], h)
    assert torch.equal(w, w0 + D)


def test_device_coefficients_are_the_host_functions_bits():
    """u = 0 and K_j = the j-th unit vector of each row: element j of an interpolated output is fma(c_j, 1, 0) = c_j itself, so
    the device's h beta_j(theta) (fp64) is compared with the host form of the same text bit for bit."""
    dtype = torch.float64
    B, d = 192, 8
    ops = _ops(dtype, B * d)
    dev = ops.device
    cols, P = _table()
    nk = len(cols)
    times, cat, log_d, tnew, hit0, nxt0 = _draw(B, shift=0)
    rng_h, hit_h, _, coef = _host_plan(B, times, log_d, tnew, hit0, nxt0, nk, P)
    u = torch.zeros(B * d, dtype=dtype, device=dev)
    Ks = []
    for j in range(nk):
        k = torch.zeros(B, d, dtype=dtype, device=dev)
        k[:, j] = 1.0
        Ks.append(k.view(-1))
    sol = torch.full((T, B * d), float("nan"), dtype=dtype, device=dev)
    ops.rows_dense_eval(B, d, sol, times.to(dev), u, Ks, P, u, log_d.to(dev), tnew.to(dev), hit0.to(dev), nxt0.to(dev),
                        torch.zeros(2, B, dtype=torch.int32, device=dev))
    got = sol.view(T, B, d).cpu()
    seen = 0
    for o in range(1, T - 1):
        m = (rng_h[0] <= o) & (o < rng_h[1])
        if m.any():
            assert torch.equal(got[o, m][:, :nk], coef[o, m]), o
            seen += int(m.sum())
    assert seen > B


# ------------------------------------------------------------------ end to end
TIMES = (0.0, 0.03, 0.05, 0.1, 0.12, 0.17, 0.2)


def _spread(Bn, dtype=torch.float64):
    g = torch.Generator().manual_seed(0)
    r = torch.logspace(-1.3, 0.3, Bn, dtype=torch.float64)
    ang = 6.28 * torch.rand(Bn, generator=g, dtype=torch.float64)
    return torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=1).to(dtype)


def _solve(y0, dev, rk="5dp", tol=1e-8, backend=None, times=TIMES):
    from problems import SpiralTruth, flat_grads
    from pnode_amd import options, petsc_adjoint
    options.clear()
    options.set_option("ts_rk_type", rk)
    options.set_option("ts_rtol", tol)
    options.set_option("ts_atol", tol)
    options.set_option("pn_adapt_scope", "sample")
    options.set_option("pn_output_times", "interpolate")
    try:
        f = SpiralTruth(y0.dtype).to(dev)
        ode = petsc_adjoint.ODEPetsc(backend=backend) if backend is not None else petsc_adjoint.ODEPetsc()
        y = y0.to(dev).clone().requires_grad_(True)
        ode.setupTS(y, f, step_size=0.01, method="dopri5")
        pred = ode.odeint_adjoint(y, torch.tensor(times, dtype=torch.float64, device=dev))
        # per-row weights that travel with the row (a function of its initial state): slicing or permuting the batch keeps them
        w0 = (1.0 + 0.3 * torch.sin(7.0 * y0.double())).to(pred.dtype).to(dev)
        w = torch.stack([w0 * (1.0 + 0.1 * i) for i in range(pred.shape[0])])
        (pred * w).sum().backward()
        return pred.detach().cpu(), y.grad.cpu(), flat_grads(f).cpu(), ode
    finally:
        options.clear()


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())


@pytest.mark.parametrize("rk", ["3bs", "5dp"])
def test_device_solve_equals_the_cpu_stand_in(rk):
    from _cpu_rows_dense_ops import CpuRowsDenseOps
    dev = require_gpu()
    tol = {"3bs": 1e-6, "5dp": 1e-8}[rk]
    y0 = _spread(6)
    sol, gu, gp, ode = _solve(y0, dev, rk, tol)
    rsol, rgu, rgp, rode = _solve(y0, torch.device("cpu"), rk, tol, backend=CpuRowsDenseOps)
    assert torch.equal(ode.sample_steps, rode.sample_steps) and torch.equal(ode.sample_rejections, rode.sample_rejections)
    assert ode.rounds == rode.rounds and int(ode.sample_steps.max()) >= 2 * int(ode.sample_steps.min())
    worst = max(_rel(sol, rsol), _rel(gu, rgu), _rel(gp, rgp))
    print("sample mode with interpolated outputs, %s: device against the CPU stand-in %.2e" % (rk, worst))
    assert worst <= 1e-11


def test_rows_do_not_depend_on_the_batch_on_the_device():
    dev = require_gpu()
    y0 = _spread(8)
    sol, gu, _, ode = _solve(y0, dev)
    hsol, hgu, _, hode = _solve(y0[4:], dev)
    assert torch.equal(sol[:, 4:], hsol) and torch.equal(gu[4:], hgu) and torch.equal(ode.sample_steps[4:], hode.sample_steps)
    perm = [3, 0, 5, 1, 7, 4, 2, 6]
    psol, pgu, _, _ = _solve(y0[perm], dev)
    assert torch.equal(sol[:, perm], psol) and torch.equal(gu[perm], pgu)
    sol2, gu2, _, _ = _solve(y0, dev)
    assert torch.equal(sol, sol2) and torch.equal(gu, gu2)
