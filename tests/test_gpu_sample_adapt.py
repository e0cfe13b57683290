"""-m gpu: the pn_rows_* kernels (csrc/pn_rows.hip) against fp64 host arithmetic, and -pn_adapt_scope sample end to end on the
device against the CPU stand-in (tests/_cpu_rows_ops.py)."""
import ctypes

import pytest
import torch

from conftest import require_gpu
from pnode_amd import _lib

pytestmark = pytest.mark.gpu

DS = [1, 2, 5, 512, 4099, 2 ** 16 + 3]
BS = [1, 3, 4096]
FITS = 2 ** 25            # B * d elements per vector of a kernel test: 4096 x (2^16 + 3) is left out (its vectors are drawn on the
                          # host, a quarter of a billion numbers each), 4096 x 4099 is in
STRIDE = (9000, 512)      # more row groups than the capped grid has workgroups (fp32: 2 rows per workgroup, 4500 > 4096):
                          # every kernel takes a second trip of its block-stride loop


def _ops(dtype, n):
    from pnode_amd.petsc_adjoint import HipVecOps
    return HipVecOps(require_gpu(), dtype, n)


def _tol(dtype):
    return 2e-6 if dtype == torch.float32 else 1e-14


def _vecs(B, d, dtype, k, dev, offset=0, seed=0):
    g = torch.Generator().manual_seed(B * 131 + d * 7 + k + seed)
    return [torch.randn(B * d + offset, generator=g, dtype=dtype).to(dev)[offset:] for _ in range(k)]


def _h(B, dev, seed=1, zeros=True):
    g = torch.Generator().manual_seed(seed + B)
    h = 0.05 + 0.2 * torch.rand(B, generator=g, dtype=torch.float64)
    if zeros and B > 1:
        h[::3] = 0.0            # rejected / finished rows ride along with h = 0
    return h.to(dev)


def _shapes():
    return [(B, d) for d in DS for B in BS if B * d <= FITS] + [STRIDE]


def _close(a, b, dtype):
    return torch.allclose(a.double(), b, rtol=_tol(dtype), atol=_tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,d", _shapes())
@pytest.mark.parametrize("offset", [0, 1])
def test_rows_stage_and_adj_theta(dtype, B, d, offset):
    ops = _ops(dtype, B * d)
    dev = ops.device
    u, k1, k2, k3 = _vecs(B, d, dtype, 4, dev, offset)
    h = _h(B, dev)
    coef = [0.3, -0.7, 1.1]
    y = torch.full((B * d + offset,), float("nan"), dtype=dtype, device=dev)[offset:]
    ops.rows_stage(B, d, y, u, [k1, k2, k3], coef, h)
    hb = h.view(B, 1)
    ref = u.double().view(B, d).clone()
    for c, k in zip(coef, (k1, k2, k3)):
        ref = ref + (hb * c) * k.double().view(B, d)
    assert _close(y.view(B, d), ref, dtype)
    if B > 1:
        assert torch.equal(y.view(B, d)[0], u.view(B, d)[0])          # h = 0: the stage value is the state, bit for bit
    y2 = torch.empty_like(y)
    ops.rows_stage(B, d, y2, u, [k1, k2, k3], coef, h)
    assert torch.equal(y, y2)
    # a row is the bits of pn_rk_stage with the same h
    one = _ops(dtype, d)
    for r in sorted({0, B // 2, B - 1}):
        yr = torch.empty(d, dtype=dtype, device=dev)
        hr = float(h[r])
        one.rk_stage(yr, u.view(B, d)[r].clone(), [k.view(B, d)[r].clone() for k in (k1, k2, k3)], [hr * c for c in coef])
        assert torch.equal(yr, y.view(B, d)[r])
    # cotangent form: the first term is a product
    w = torch.empty_like(y)
    ops.rows_adj_theta(B, d, w, u, 0.4, [k1, k2], [0.3, -0.7], h)
    ref = (hb * 0.4) * u.double().view(B, d) + (hb * 0.3) * k1.double().view(B, d) + (hb * -0.7) * k2.double().view(B, d)
    assert _close(w.view(B, d), ref, dtype)
    ops.rows_adj_theta(B, d, w, None, 0.0, [k1, k2], [0.3, -0.7], h)
    ref = (hb * 0.3) * k1.double().view(B, d) + (hb * -0.7) * k2.double().view(B, d)
    assert _close(w.view(B, d), ref, dtype)
    w2 = torch.empty_like(w)
    ops.rows_adj_theta(B, d, w2, None, 0.0, [k1, k2], [0.3, -0.7], h)
    assert torch.equal(w, w2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,d", _shapes())
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("fsal", [False, True])
def test_rows_combine_wrms(dtype, B, d, offset, fsal):
    ops = _ops(dtype, B * d)
    dev = ops.device
    u, k1, k2 = _vecs(B, d, dtype, 3, dev, offset)
    h = _h(B, dev, zeros=False)
    cb, ce = [0.6, 0.4], [1e-3, -2e-3]
    atol, rtol = 1e-5, 1e-4
    unew = None if fsal else torch.full((B * d + offset,), float("nan"), dtype=dtype, device=dev)[offset:]
    enorm = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    ops.rows_combine_wrms(B, d, unew, u, [k1, k2], cb, ce, h, atol, rtol, enorm)
    hb = h.view(B, 1)
    un = u.double().view(B, d).clone()
    if not fsal:
        for c, k in zip(cb, (k1, k2)):
            un = un + (hb * c) * k.double().view(B, d)
        assert _close(unew.view(B, d), un, dtype)
        un = unew.double().view(B, d)
    # the stored uhat: err as the kernel's chain forms it, fma((T)(h_r ce_j), K_j, err) -- fp32 products are exact in fp64, one
    # rounding per step -- so for fp32 states only the rounding of tol and of the quotient is left (5e-7; the exact-operand cases
    # of tests/test_gpu_error_norm.py are the sharp ones)
    err = torch.zeros_like(un)
    for c, k in zip(ce, (k1, k2)):
        err = ((hb * c).to(dtype).double() * k.double().view(B, d) + err).to(dtype).double()
    uh = (un + err).to(dtype).double()
    ref = ((((un - uh) / (atol + rtol * torch.maximum(un.abs(), uh.abs()))) ** 2).sum(1) / d).sqrt()
    assert torch.allclose(enorm, ref, rtol=1e-6 if dtype == torch.float32 else 1e-9, atol=1e-12)
    e2 = torch.empty_like(enorm)
    ops.rows_combine_wrms(B, d, None if fsal else torch.empty_like(unew), u, [k1, k2], cb, ce, h, atol, rtol, e2)
    assert torch.equal(enorm, e2)
    if B > 1:
        # a row's norm does not depend on the batch it is in, nor on its position: the second half alone, bit for bit
        lo = B // 2
        sub = _ops(dtype, (B - lo) * d)
        e3 = torch.empty(B - lo, dtype=torch.float64, device=dev)
        sub.rows_combine_wrms(B - lo, d, None if fsal else torch.empty((B - lo) * d, dtype=dtype, device=dev),
                              u.view(B, d)[lo:].reshape(-1).clone(), [k.view(B, d)[lo:].reshape(-1).clone() for k in (k1, k2)],
                              cb, ce, h[lo:].clone(), atol, rtol, e3)
        assert torch.equal(enorm[lo:], e3)


def _matrix(T, n, dtype, dev, offset, pad, seed):
    """T rows of n elements with row stride n + pad, the first row `offset` elements into its storage."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(offset + T * (n + pad), generator=g, dtype=dtype).to(dev)
    return base[offset:].view(T, n + pad)[:, :n]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,d", _shapes())
@pytest.mark.parametrize("mask", ["random", "none", "all"])
@pytest.mark.parametrize("layout", ["aligned", "bases+1", "matrix+1", "ld+1"])
def test_rows_commit_and_adj_accum(dtype, B, d, mask, layout):
    """layout: every base 16-byte aligned; the vectors one element off; only the solution / cotangent matrix one element off;
    only its row stride not a multiple of the vector width -- each must send the launch to the scalar form."""
    ops = _ops(dtype, B * d)
    dev = ops.device
    T = 3
    n = B * d
    off = 1 if layout == "bases+1" else 0
    moff, pad = (1 if layout == "matrix+1" else 0), (1 if layout == "ld+1" else 0)
    u, unew, x1, x2 = _vecs(B, d, dtype, 4, dev, off)
    g = torch.Generator().manual_seed(B + d)
    acc = {"random": torch.randint(0, 2, (B,), generator=g), "none": torch.zeros(B, dtype=torch.int64),
           "all": torch.ones(B, dtype=torch.int64)}[mask].to(torch.int32).to(dev)
    hit = (torch.randint(0, T + 1, (B,), generator=g) - 1).to(torch.int32).to(dev)
    sol = _matrix(T, n, dtype, dev, moff, pad, 3)
    sol.zero_()
    ld = sol.stride(0)
    gaps = sol.as_strided((T,), (ld,), n).clone() if pad else None        # what lies between the rows stays as it was
    assert ld == n + pad and (sol.data_ptr() % 16 != 0) == bool(moff)
    nxt = torch.full((n + off,), float("nan"), dtype=dtype, device=dev)[off:]
    ops.rows_commit(B, d, nxt, u, unew, acc, hit, sol, ld, T)
    a = acc.bool().view(B, 1)
    assert torch.equal(nxt.view(B, d), torch.where(a, unew.view(B, d), u.view(B, d)))
    ref = torch.zeros(T, B, d, dtype=dtype, device=dev)
    for i in range(T):
        m = (a.view(B) & (hit == i)).view(B, 1)
        ref[i] = torch.where(m, unew.view(B, d), ref[i])
    assert torch.equal(sol.reshape(T, B, d), ref)
    if pad:
        assert torch.equal(sol.as_strided((T,), (ld,), n), gaps)
    nxt2, sol2 = torch.empty_like(nxt), torch.zeros_like(sol)
    ops.rows_commit(B, d, nxt2, u, unew, acc, hit, sol2, sol2.stride(0), T)
    assert torch.equal(nxt, nxt2) and torch.equal(sol2, sol)
    inplace = u.clone()
    ops.rows_commit(B, d, inplace, inplace, unew, acc, hit, None, 0, 0)
    assert torch.equal(inplace, nxt)
    # lam + x1 + x2 + g[hit]
    gg = _matrix(T, n, dtype, dev, moff, pad, 5)
    out = torch.full((n + off,), float("nan"), dtype=dtype, device=dev)[off:]
    ops.rows_adj_accum(B, d, out, u, [x1, x2], gg, gg.stride(0), hit, T)
    ref = u.double().view(B, d) + x1.double().view(B, d) + x2.double().view(B, d)
    for i in range(T):
        ref = ref + torch.where((hit == i).view(B, 1), gg[i].double().view(B, d), torch.zeros_like(ref))
    assert _close(out.view(B, d), ref, dtype)
    out2 = u.clone()
    ops.rows_adj_accum(B, d, out2, out2, [x1, x2], gg, gg.stride(0), hit, T)           # in place, and run to run
    assert torch.equal(out, out2)
    if layout != "aligned":
        # the scalar form walks the same chunks: the same bits as the vector form on aligned copies
        al = torch.empty(n, dtype=dtype, device=dev)
        ga = gg.contiguous()
        ops.rows_adj_accum(B, d, al, u.clone(), [x1.clone(), x2.clone()], ga, n, hit, T)
        assert torch.equal(al, out)
    ops.rows_adj_accum(B, d, out2, u, [], None, 0, None, 0)
    assert torch.equal(out2, u)


@pytest.mark.parametrize("B", [1, 3, 300, 4096, 70000])        # 70000: more workgroups than the last one has threads
@pytest.mark.parametrize("case", ["random", "all-rejected", "all-finished", "nan-row"])
@pytest.mark.parametrize("nspan", [0, 4])
def test_rows_control_is_the_host_controller(B, case, nspan):
    dev = require_gpu()
    lib = _lib.load()
    ops = _ops(torch.float64, B)
    ts = ctypes.c_void_p(lib.pn_ts_create())
    _lib.check(lib.pn_ts_set_rk_type(ts, b"5dp"))
    g = torch.Generator().manual_seed(B + nspan)
    span = torch.tensor([0.0, 0.1, 0.25, 0.4], dtype=torch.float64)
    tmax = 0.4
    sd = torch.zeros(_lib.PN_ROWS_ND, B, dtype=torch.float64)
    sd[_lib.PN_ROWS_T] = 0.1 * torch.rand(B, generator=g, dtype=torch.float64)
    sd[_lib.PN_ROWS_H] = 0.001 + 0.05 * torch.rand(B, generator=g, dtype=torch.float64)
    sd[_lib.PN_ROWS_TFIRST] = sd[_lib.PN_ROWS_T]
    si = torch.zeros(_lib.PN_ROWS_NI, B, dtype=torch.int32)
    if nspan:
        si[_lib.PN_ROWS_SPANCTR] = 1
    enorm = torch.exp(2.0 * torch.randn(B, generator=g, dtype=torch.float64)) * 0.5
    if case == "all-rejected":
        enorm = enorm + 1.5
    if case == "all-finished":
        si[_lib.PN_ROWS_FINISHED] = 1
    if case == "nan-row":
        enorm[B // 2] = float("nan")
    outs = []
    for where in ("host", "device", "device"):
        to = (lambda x: x.clone()) if where == "host" else (lambda x: x.to(dev))
        s_d, s_i, en = to(sd), to(si), to(enorm)
        log_d = to(torch.full((3, B), -7.0, dtype=torch.float64))
        log_hit, accept, summary = to(torch.full((B,), -7, dtype=torch.int32)), to(torch.full((B,), -7, dtype=torch.int32)), to(torch.zeros(4, dtype=torch.int32))
        sp = to(span) if nspan else None
        for _ in range(3):                     # three rounds on the same error norms
            if where == "host":
                _lib.check(lib.pn_rows_control_host(ts, B, nspan, None if sp is None else sp.data_ptr(), tmax, en.data_ptr(), s_d.data_ptr(),
                                                    s_i.data_ptr(), log_d.data_ptr(), log_hit.data_ptr(), accept.data_ptr(), summary.data_ptr()))
            else:
                ops.rows_control(ts, B, nspan, sp, tmax, en, s_d, s_i, log_d, log_hit, accept, summary)
        outs.append([x.cpu() for x in (s_d, s_i, log_d, log_hit, accept, summary)])
    lib.pn_ts_destroy(ts)
    host, device, again = outs
    assert all(torch.equal(x, y) or (torch.isnan(x) == torch.isnan(y)).all() and torch.equal(x.nan_to_num(), y.nan_to_num())
               for x, y in zip(device, again))                    # bitwise run to run
    for k in (1, 3, 4, 5):
        assert torch.equal(host[k], device[k]), k
    for k in (0, 2):                            # pow on the device and in libm may differ in the last bits
        assert torch.allclose(host[k], device[k], rtol=1e-14, atol=0.0, equal_nan=True), k
    if case == "all-finished":
        assert int(device[5][0]) == 0 and int(device[4].sum()) == 0 and float(device[2][0].abs().max()) == 0.0
    if case == "all-rejected":
        assert int(device[4].sum()) == 0
    if case == "nan-row":
        assert int(device[5][1]) == B // 2 and int(device[5][2]) == 1


# ------------------------------------------------------------------ end to end
def _spread(Bn, dtype=torch.float64):
    g = torch.Generator().manual_seed(0)
    r = torch.logspace(-1.3, 0.3, Bn, dtype=torch.float64)
    ang = 6.28 * torch.rand(Bn, generator=g, dtype=torch.float64)
    return torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=1).to(dtype)


def _solve(y0, dev, rk="5dp", tol=1e-8, backend=None, func=None, times=(0.0, 0.05, 0.12, 0.2)):
    from problems import SpiralTruth, flat_grads
    from pnode_amd import options, petsc_adjoint
    options.clear()
    options.set_option("ts_rk_type", rk)
    options.set_option("ts_rtol", tol)
    options.set_option("ts_atol", tol)
    options.set_option("pn_adapt_scope", "sample")
    try:
        f = (SpiralTruth(y0.dtype) if func is None else func).to(dev)
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


@pytest.mark.parametrize("rk", ["3bs", "5dp", "5f", "2a"])
def test_device_solve_equals_the_cpu_stand_in(rk):
    from _cpu_rows_ops import CpuRowsOps
    dev = require_gpu()
    tol = {"3bs": 1e-6, "5dp": 1e-8, "5f": 1e-8, "2a": 1e-4}[rk]
    y0 = _spread(6)
    sol, gu, gp, ode = _solve(y0, dev, rk, tol)
    rsol, rgu, rgp, rode = _solve(y0, torch.device("cpu"), rk, tol, backend=CpuRowsOps)
    assert torch.equal(ode.sample_steps, rode.sample_steps) and torch.equal(ode.sample_rejections, rode.sample_rejections)
    assert ode.rounds == rode.rounds and int(ode.sample_steps.max()) >= 2 * int(ode.sample_steps.min())
    worst = max(_rel(sol, rsol), _rel(gu, rgu), _rel(gp, rgp))
    print("sample mode, %s: device against the CPU stand-in %.2e" % (rk, worst))
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
    sol2, gu2, gp2, _ = _solve(y0, dev)
    assert torch.equal(sol, sol2) and torch.equal(gu, gu2)


def test_fp32_at_4096_x_512_against_the_fp64_engine():
    """The project's bar for fp32 states (tests/test_gpu_configs.py): dL/dtheta within 1e-5 relative of the fp64 engine run with the
    same options."""
    from problems import MLPFunc
    dev = require_gpu()
    g = torch.Generator().manual_seed(3)
    y0 = torch.randn(4096, 512, generator=g, dtype=torch.float64) * torch.logspace(-1, 0.5, 4096, dtype=torch.float64).view(-1, 1)
    times = (0.0, 0.5, 1.0)
    out = {}
    for dt in (torch.float32, torch.float64):
        f = MLPFunc(512, dt, std=0.05)
        sol, gu, gp, ode = _solve(y0.to(dt), dev, "5dp", 1e-4, func=f, times=times)
        out[dt] = (sol, gu, gp, ode)
    s32, s64 = out[torch.float32], out[torch.float64]
    print("4096 x 512: rounds fp32 %d fp64 %d; dL/dtheta fp32 against fp64 %.2e; states %.2e"
          % (s32[3].rounds, s64[3].rounds, _rel(s32[2], s64[2]), _rel(s32[0], s64[0])))
    assert _rel(s32[2], s64[2]) <= 1e-5
