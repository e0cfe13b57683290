"""-m gpu: the row-compaction kernels of csrc/pn_rows.hip (pn_rows_list, pn_rows_gather, pn_rows_scatter) against the host twin and
torch indexing, compared as integers so that NaN payloads and -0.0 count, and -pn_rows_compact 1 against 0 in whole solves on the
device.  The batches, funcs and bounds are those of tests/test_rows_compact.py."""
import pytest
import torch

import _rows_compact_cases as C
from conftest import require_gpu
from pnode_amd import _lib
from test_rows_compact import check_list, list_patterns, list_source

pytestmark = pytest.mark.gpu

INT = {torch.float32: torch.int32, torch.float64: torch.int64}


def _ops(dtype, n=1):
    from pnode_amd._vecops import HipVecOps
    return HipVecOps(require_gpu(), dtype, n)


# ---------------------------------------------------------------------------------------------------- the list
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 100003])
def test_rows_list_is_the_host_twins_list(kind, n):
    dev = require_gpu()
    ops, lib = _ops(torch.float64), _lib.load()
    cases = list(list_patterns(n).items())
    if kind == 1:
        cases.append(("nan", [r != n // 2 for r in range(n)]))
    for name, listed in cases:
        src = list_source(kind, listed, nan_at=n // 2 if name == "nan" else None)
        hidx, hpos, hcount = (torch.full((k,), 77, dtype=torch.int32) for k in (n, n, 1))
        _lib.check(lib.pn_rows_list_host(n, kind, src.data_ptr(), hidx.data_ptr(), hpos.data_ptr(), hcount.data_ptr()))
        if n <= 1025:
            check_list(listed, hidx, hpos, hcount)
        got = []
        for fill in (77, -5):                                 # two launches over buffers that held different things: the same bytes
            idx, pos, count = (torch.full((k,), fill, dtype=torch.int32, device=dev) for k in (n, n, 1))
            ops.rows_list(n, kind, src.to(dev), idx, pos, count)
            got.append((idx.cpu(), pos.cpu(), count.cpu()))
        for idx, pos, count in got:
            assert torch.equal(count, hcount), (name, count, hcount)
            assert torch.equal(idx, hidx) and torch.equal(pos, hpos), name


# ---------------------------------------------------------------------------------------------------- the two copies
def _bits(rows, d, dtype, seed):
    """rows x d values of every kind: random bit patterns (NaNs with payloads, infinities, denormals among them), -0.0 and a quiet NaN"""
    g = torch.Generator().manual_seed(seed)
    it = INT[dtype]
    info = torch.iinfo(it)
    x = torch.randint(info.min, info.max, (rows, d), generator=g, dtype=it)
    if rows * d > 2:
        x.view(-1)[1] = info.min                              # -0.0
        x.view(-1)[2] = torch.tensor(float("nan"), dtype=dtype).view(it)
    return x


def _place(x, dev, offset, dtype):
    """the integer matrix x as a flat device tensor of `dtype` whose base is 16-byte aligned (offset 0) or one element past that"""
    buf = torch.empty(x.numel() + 4, dtype=INT[dtype], device=dev)
    flat = buf[offset: offset + x.numel()]
    flat.copy_(x.reshape(-1))
    assert flat.data_ptr() % 16 == (0 if offset == 0 else flat.element_size())
    return flat.view(dtype)


def _subset(B, m, seed):
    g = torch.Generator().manual_seed(seed)
    return sorted(torch.randperm(B, generator=g)[:m].tolist())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 64, 513])
def test_rows_gather_and_scatter_move_bits(dtype, d):
    dev = require_gpu()
    ops = _ops(dtype)
    it = INT[dtype]
    nan = torch.tensor(float("nan"), dtype=dtype)
    for B in (1, 2, 65, 1000, 4097):
        for m in sorted(set((0, 1, B // 3, B))):
            rows = _subset(B, m, seed=B + m)
            idx = torch.tensor(rows + [-1] * (B - m), dtype=torch.int32)
            pos = torch.full((B,), -1, dtype=torch.int32)
            pos[rows] = torch.arange(m, dtype=torch.int32)
            listed = torch.zeros(B, dtype=torch.bool)
            listed[rows] = True
            for offset in (0, 1):
                # gather: the unlisted rows of the source hold NaN and leave no trace
                src = _bits(B, d, dtype, seed=d + B)
                src[~listed] = nan.view(it)
                out = _place(torch.full((max(m, 1), d), 0x55, dtype=it), dev, offset, dtype)
                ops.rows_gather(m, d, out, _place(src, dev, offset, dtype), idx.to(dev))
                assert torch.equal(out.view(it).cpu()[: m * d].view(m, d), src[rows]), ("gather", B, m, offset)
                if m >= 2:                                    # a stale list: a -1 inside the first m entries is a row of zeros
                    hole = idx.clone()
                    hole[m // 2] = -1
                    ops.rows_gather(m, d, out, _place(src, dev, offset, dtype), hole.to(dev))
                    want = src[rows].clone()
                    want[m // 2] = 0
                    assert torch.equal(out.view(it).cpu()[: m * d].view(m, d), want), ("gather hole", B, m, offset)
                # scatter: every row of a target full of NaN is written; the source's rows past the list hold NaN
                sub = _bits(B, d, dtype, seed=d + B + 1)
                sub[m:] = nan.view(it)
                full = _place(nan.view(it).expand(B, d).contiguous(), dev, offset, dtype)
                ops.rows_scatter(B, d, full, _place(sub, dev, offset, dtype), pos.to(dev))
                want = torch.zeros(B, d, dtype=it)            # (integer zero: +0.0)
                want[rows] = sub[:m]
                assert torch.equal(full.view(it).cpu().view(B, d), want), ("scatter", B, m, offset)
    # the rows' times: fp64, one entry per row, whatever the state's dtype
    tv = torch.rand(65, dtype=torch.float64)
    rows = _subset(65, 20, 0)
    tc = torch.empty(20, dtype=torch.float64, device=dev)
    ops.rows_gather(20, 1, tc, tv.to(dev), torch.tensor(rows, dtype=torch.int32, device=dev))
    assert torch.equal(tc.cpu(), tv[rows])


# ---------------------------------------------------------------------------------------------------- whole solves on the device
def _same_counts(a, b):
    oa, ob = a["ode"], b["ode"]
    assert torch.equal(oa.sample_steps, ob.sample_steps) and torch.equal(oa.sample_rejections, ob.sample_rejections)
    assert oa.rounds == ob.rounds and oa.nfe_forward == ob.nfe_forward


def _cpu(out):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def test_fp64_mlp_on_a_spread_batch_on_the_device():
    from _cpu_rows_compact_ops import CpuRowsCompactOps
    dev = require_gpu()
    off, on = (_cpu(C.solve(None, c, func="mlp", B=8, device=dev)) for c in ("0", "1"))
    steps = off["ode"].sample_steps
    assert int(steps.min()) <= int(steps.max()) / 2
    _same_counts(off, on)
    for la, lb in zip(off["logs"], on["logs"]):
        assert len(la) == len(lb)
        for n, ((ta, ha), (tb, hb)) in enumerate(zip(la, lb)):
            bound = (n + 1) * 2.0 ** -52 / C.TOL["5dp"]          # (tests/test_rows_compact.py's docstring)
            assert abs(ha - hb) <= bound * ha and abs(ta - tb) <= bound * C.TIMES[-1]
    worst = {key: C.rel(on[key], off[key]) for key in ("sol", "gu", "gp")}
    print("device, mlp: 1 against 0 %s; rows evaluated %s" % (worst, on["ode"].rows_compact))
    assert max(worst.values()) <= 1e-12, worst
    assert on["ode"].rows_evaluated < 0.75 * off["ode"].rows_evaluated
    assert off["ode"].rows_evaluated == 8 * off["ode"].nfe_forward and off["ode"].rows_compact == "off"
    # and against the CPU stand-in under 1: tests/test_gpu_sample_adapt.py's tolerance for that pair
    ref = C.solve(CpuRowsCompactOps, "1", func="mlp", B=8)
    _same_counts(on, ref)
    assert on["ode"].rows_evaluated == ref["ode"].rows_evaluated
    assert on["ode"].rows_evaluated_backward == ref["ode"].rows_evaluated_backward
    worst = max(C.rel(on[key], ref[key]) for key in ("sol", "gu", "gp"))
    print("device against the CPU stand-in, both compacted: %.2e" % worst)
    assert worst <= 1e-11


FP32_TIMES = [0.0, 0.3, 0.6, 1.0]


def test_fp32_row_independent_func_gives_the_same_bits_on_the_device():
    """fp32 states, the spiral in elementwise operations (a row's bits cannot depend on the row count): the solution and dL/dy0 are
    the same bits.  dL/dA is, per func call, a sum over the rows func was given: m terms under 1, the same m terms and B - m exact
    zeros under 0, added by the library's reduction in an order that depends on the count -- round-off of fp32, not bits.  Its bound
    is the project's bar for dL/dtheta of fp32 states, 1e-5 relative (tests/test_gpu_sample_adapt.py, tests/test_gpu_configs.py);
    the figure is printed."""
    dev = require_gpu()
    kw = dict(func="elementwise", B=16, tol=1e-4, times=FP32_TIMES, device=dev, dtype=torch.float32)
    off, on = (_cpu(C.solve(None, c, **kw)) for c in ("0", "1"))
    _same_counts(off, on)
    assert int(off["ode"].sample_steps.min()) * 2 <= int(off["ode"].sample_steps.max()), off["ode"].sample_steps
    assert off["logs"] == on["logs"]
    for key in ("sol", "gu"):
        assert torch.equal(off[key], on[key]), (key, C.rel(on[key], off[key]))
    print("device, fp32 elementwise spiral: dL/dA 1 against 0 %.2e (equal: %s); %s"
          % (C.rel(on["gp"], off["gp"]), torch.equal(on["gp"], off["gp"]), on["ode"].rows_compact))
    assert C.rel(on["gp"], off["gp"]) <= 1e-5
    assert on["ode"].rows_evaluated < 0.75 * off["ode"].rows_evaluated
    assert on["ode"].rows_evaluated_backward < off["ode"].rows_evaluated_backward


@pytest.mark.parametrize("case", ["interpolate", "tgrad"])
def test_interpolated_outputs_and_dl_dt_on_the_device(case):
    """fp64 on the device, 1 against 0 and against the CPU stand-in under 1.  The solution and dL/dy0 are the same bits; the
    parameter gradients are sums over the rows func was given (above): 1e-12."""
    from _cpu_rows_compact_ops import CpuRowsCompactOps
    dev = require_gpu()
    kw = dict(func="spiral", B=8, extra=(("pn_output_times", "interpolate"),)) if case == "interpolate" else dict(func="time", B=8, tgrad=True)
    off, on = (_cpu(C.solve(None, c, device=dev, **kw)) for c in ("0", "1"))
    _same_counts(off, on)
    assert off["logs"] == on["logs"]
    assert torch.equal(off["sol"], on["sol"]) and torch.equal(off["gu"], on["gu"])
    print("device, %s: dL/dtheta 1 against 0 %.2e (equal: %s)" % (case, C.rel(on["gp"], off["gp"]), torch.equal(on["gp"], off["gp"])))
    assert C.rel(on["gp"], off["gp"]) <= 1e-12
    if case == "tgrad":
        assert float(off["gt"].abs().min()) > 0.0
        assert C.rel(on["gt"], off["gt"]) <= 1e-12 and C.rel(on["dtrow"], off["dtrow"]) <= 1e-12
    ref = C.solve(CpuRowsCompactOps, "1", **kw)
    _same_counts(on, ref)
    keys = ("sol", "gu", "gp") + (("gt",) if case == "tgrad" else ())
    assert max(C.rel(on[k], ref[k]) for k in keys) <= 1e-11
