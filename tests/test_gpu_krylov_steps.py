"""-m gpu: the device GMRES kernels (pnode_amd/csrc/pn_krylov.hip) launch by launch.  The host looks at the state block
after every launch (tests/_krylov_cases.py read_state) and compares it with the Python twin of the state machine on the
same inputs (decisions: exactly; numbers: within the spread between the twin and its perturbed form) and with a float64
Arnoldi (residual history, orthogonality, the Arnoldi relation, the true residual of x).  tests/test_krylov_steps.py
shows on the CPU that the cases are what they claim to be.  Every test prints its largest error-to-tolerance ratios
("RATIO ..." lines)."""
import functools

import pytest
import torch

import _krylov_cases as kc
from conftest import require_gpu

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
KEEP126 = (0, 7, 8, 63, 64, 125)


def _device_run(case, n, dtype, restart, b=None, misaligned=False, **kw):
    from pnode_amd.petsc_adjoint import HipVecOps
    dev = require_gpu()
    ops = HipVecOps(dev, dtype, n)
    A, b0 = kc.operator(case, n)
    b = b0 if b is None else b
    if misaligned:                     # views one element into larger buffers: not 16-byte aligned; guards of 7.0 around them
        rbuf = torch.full((n + 2,), 7.0, dtype=dtype, device=dev)
        xbuf = torch.full((n + 2,), 7.0, dtype=dtype, device=dev)
        rhs, x = rbuf[1: n + 1], xbuf[1: n + 1]
        rhs.copy_(b.to(dtype))
        assert rhs.data_ptr() % 16 and x.data_ptr() % 16
    else:
        rbuf = xbuf = None
        rhs, x = b.to(dtype).to(dev), torch.zeros(n, dtype=dtype, device=dev)
        assert rhs.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    run = kc.Run(ops, A.to(dtype).to(dev), rhs, x, restart, **kw)
    run.rbuf, run.xbuf = rbuf, xbuf
    return run


def _scripted(case, n, dtype, restart, steps, steps2, keep=None, **kw):
    """The script of the issue on the device: `steps` columns, a close, a second cycle of `steps2` columns from
    r = b - A x with first=False.  Returns (run, trace of cycle 1, residual on the host, trace of cycle 2)."""
    run = _device_run(case, n, dtype, restart, keep=keep, **kw)
    rtol = 1e-30 if case == "slow" else kc.solve_rtol(n, restart, dtype)
    run.cycle(run.rhs, steps, rtol, 1e-50, 10000, True)
    first, run.trace = run.trace, []
    r = run.residual()
    run.cycle(r, steps2, 0.0, 0.0, 0, False, close=False)
    return run, first, r.cpu(), run.trace


@functools.lru_cache(maxsize=None)
def _explicit(case, n, dtype):
    """The plain form (explicit k, decisions in the product kernel) of the restart-12 script: run once, shared."""
    return _scripted(case, n, dtype, 12, 12, 3)


class _Trace(object):
    def __init__(self, run, trace):
        self.trace, self.kr = trace, run.kr


def _against_twin_and_reference(label, dtype, case, n, restart, steps, steps2, dev, keep=None, b=None):
    """The assertions of group 1 on a finished device script."""
    run, first, r, second = dev
    if b is None:
        tw, pt = kc.twins(case, n, dtype, restart, steps, keep)
        ref = kc.reference(case, n, dtype, restart)
    else:
        rtol = kc.solve_rtol(n, restart, dtype)
        tw, pt = (kc.twin_run(case, n, dtype, restart, p, steps, rtol, keep=keep, b=b) for p in (False, True))
        ref = kc.Reference(kc.operator(case, n)[0].to(dtype).double(), b.to(dtype).double(), min(restart, n))
    R = kc.Ratios(dtype)
    exact = kc.compare(R, _Trace(run, first), tw, pt, ref, ref.A, ref.b, "cycle 1")
    assert not exact, exact
    # the second cycle starts from the residual the DEVICE computed: an input of begin, the same for all three
    tw2, pt2 = kc.second_cycle(tw, r, steps2), kc.second_cycle(pt, r, steps2)
    ref2 = kc.Reference(ref.A, r.double(), min(steps2, n))
    exact = kc.compare(R, _Trace(run, second), tw2, pt2, ref2, ref.A, r.double(), "cycle 2")
    assert not exact, exact
    R.check("%s %s n=%d %s" % (label, case, n, str(dtype).replace("torch.", "")))
    return tw


def _same_bits(a, b, n, what, first=False):
    for sa, sb in zip(a, b):
        where = "%s after %s %d" % (what, sa.what, sa.k)
        assert torch.equal(sa.st["raw"].view(torch.int64), sb.st["raw"].view(torch.int64)), where + ": state block"
        rows = sa.st["kdone"] + (1 if sa.st["stop"] == 0 else 0)           # the vectors of the cycle written so far
        assert torch.equal(sa.V[:rows, :n], sb.V[:rows, :n]), where + ": V"
        for name in ("vin", "x") if first and sa.what == "begin" else ("vin", "w", "x"):   # (w: nothing has written it yet)
            assert torch.equal(getattr(sa, name)[:n], getattr(sb, name)[:n]), where + ": " + name
    assert len(a) == len(b)


# ---- 1. column by column
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 257, 1031, 4099])
@pytest.mark.parametrize("case", ["plain", "near", "mixed", "open"])
def test_every_launch_against_the_twin_and_float64(case, n, dtype):
    """Restart 12: begin, 12 steps, close, begin(first=False), 3 steps; the state block, V, vin and x after every launch.
    plain and near take the second pass on every column (kr_update mode 1 in place, kr_dots mode 2, the refined column
    d + d2, kr_update mode 2), open on none, mixed on some."""
    tw = _against_twin_and_reference("columns", dtype, case, n, 12, 12, 3, _explicit(case, n, dtype))
    run, first, _, _ = _explicit(case, n, dtype)
    done = first[-1].st
    assert done["second_passes"] == tw.trace[-1].st["second_passes"] and done["ticket"].view(torch.int64).eq(0).all()
    if case in ("plain", "near"):
        assert done["second_passes"] == done["total"] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_tie_in_the_second_pass_rule_goes_to_the_second_pass(dtype):
    """rest = ww / 4 exactly (w = (3, 1, 1, 1, 0) against V_0 = e_0): `rest > 0.25 ww` is false, the column is refined."""
    dev = _scripted("tie", 5, dtype, 4, 1, 1)
    assert dev[1][1].st["phase"] == 3 and dev[1][1].st["second_passes"] == 1 and dev[1][1].st["hk1"] == 3.0 ** 0.5
    _against_twin_and_reference("tie", dtype, "tie", 5, 4, 1, 1, dev)


# ---- 2. full length
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [160, 1031])
def test_the_longest_legal_cycle(n, dtype):
    """Restart 126 (the closing kernel's 67 KB of LDS, 16 product groups, a coefficient table of 127 entries): all 126
    columns, the close, a restart and 4 more columns.  Scalars after every launch; the vectors at columns 0, 7, 8, 63, 64,
    125 and at the close."""
    dev = _scripted("slow", n, dtype, 126, 126, 4, keep=KEEP126)
    done = dev[1][-1].st
    assert (done["stop"], done["kdone"], done["total"], done["closed"], done["apply"], done["nt"]) == (0, 126, 126, 1, 1, 126)
    _against_twin_and_reference("full length", dtype, "slow", n, 126, 126, 4, dev, keep=KEEP126)


# ---- 3. the form hipGraphs replay
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("case", ["near", "mixed"])
def test_the_fused_form_leaves_the_bits_of_the_explicit_form(case, n, dtype):
    """pn_krylov_step(k = -1): the second pass takes its column from S_CUR.  After every launch the state block from the
    header to the end of y, V, vin, w and x are those of the explicit-k run bit for bit, and no arrival counter is left."""
    fused = _scripted(case, n, dtype, 12, 12, 3, fused=True)
    plain = _explicit(case, n, dtype)
    _same_bits(fused[1], plain[1], n, "cycle 1", first=True)
    _same_bits(fused[3], plain[3], n, "cycle 2")
    for s in fused[1] + fused[3]:
        assert s.st["ticket"].view(torch.int64).eq(0).all(), "an arrival counter was left non-zero"
    assert fused[1][-1].st["second_passes"] > 0
    _against_twin_and_reference("fused", dtype, case, n, 12, 12, 3, fused)


# ---- 4. the decisions as kernels of their own
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [257, 4099])
def test_deferred_decisions_leave_the_bits_of_the_fused_decisions(n, dtype):
    """reduce given (a sharded solve's form, here summing over one rank): kr_decide_kernel takes every decision, parts
    1/2 of begin and 1/2/3 of step.  Bit for bit the run whose product kernel decides."""
    deferred = _scripted("mixed", n, dtype, 12, 12, 3, reduce=lambda t: None)
    plain = _explicit("mixed", n, dtype)
    _same_bits(deferred[1], plain[1], n, "cycle 1", first=True)
    _same_bits(deferred[3], plain[3], n, "cycle 2")
    assert 0 < deferred[1][-1].st["second_passes"] < deferred[1][-1].st["total"]
    _against_twin_and_reference("deferred", dtype, "mixed", n, 12, 12, 3, deferred)


# ---- 5. the scalar form and the pad columns
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 1031])
def test_misaligned_vectors_and_untouched_pads(n, dtype):
    """rhs and x one element into larger buffers: begin and the closing update take the scalar form of kr_dots and
    kr_update.  The pad columns n..npad of V, vin and w and the guards around rhs and x hold 7.0 after every launch.
    The right-hand side is made of small integers, so <r, r> is the same in any order and the aligned solve gives the
    same bits."""
    b = kc.integer_rhs(n)

    def script(misaligned):
        run = _device_run("plain", n, dtype, 12, b=b, misaligned=misaligned)
        kr = run.kr
        kr.V[:, n:] = 7.0
        kr.vin[n:] = 7.0
        kr.w[n:] = 7.0

        def pads(s):
            where = "after %s %d" % (s.what, s.k)
            assert s.V[:, n:].eq(7.0).all() and s.vin[n:].eq(7.0).all() and s.w[n:].eq(7.0).all(), where + ": a pad was written"
            if misaligned:
                for buf in (run.rbuf, run.xbuf):
                    assert float(buf[0]) == 7.0 and float(buf[-1]) == 7.0, where + ": a guard was written"
        run.after = pads
        run.cycle(run.rhs, 12, kc.solve_rtol(n, 12, dtype), 1e-50, 10000, True)
        first, run.trace = run.trace, []
        r = run.residual()
        run.cycle(r, 3, 0.0, 0.0, 0, False, close=False)
        return run, first, r.cpu(), run.trace

    mis, ali = script(True), script(False)
    assert mis[0].kr.npad > n
    _same_bits(mis[1], ali[1], n, "cycle 1", first=True)
    _same_bits(mis[3], ali[3], n, "cycle 2")
    assert torch.equal(mis[2], ali[2])
    _against_twin_and_reference("scalar form", dtype, "plain", n, 12, 12, 3, mis, b=b)


# ---- 6. where a solve stops
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,k", [("near", 2), ("plain", 5)])
@pytest.mark.parametrize("which", ["atol", "rtol"])
def test_the_solve_stops_at_the_column_the_tolerance_asks_for(which, case, k, dtype):
    """tol = max(rtol beta, atol) at the geometric mean of rho_k and rho_{k+1} of the reference
    (tests/test_krylov_steps.py: how far every rho_j is from it): code 1 when column k + 1 is done, not before, whichever
    of the two terms gives the tolerance; with atol it is in S_TOL to the bit."""
    n = 257
    tol, _ = kc.stop_tol(case, dtype, k)
    beta = kc.reference(case, n, dtype, 12).beta
    rtol, atol = (1e-30, tol) if which == "atol" else (tol / beta, 1e-50)
    run = _device_run(case, n, dtype, 12)
    run.cycle(run.rhs, 12, rtol, atol, 10000, True)
    for s in run.trace:
        if s.what == "step":
            want = (0, s.k + 1) if s.k < k else (1, k + 1)
            assert (s.st["stop"], s.st["kdone"]) == want and s.status[:2] == want, (s.k, s.st["stop"], s.st["kdone"], s.st["res"])
    done = run.trace[-1].st
    assert (done["stop"], done["total"], done["apply"], done["closed"]) == (1, k + 1, 1, 1)
    if which == "atol":
        assert done["tol"] == atol and done["atol"] == atol
    else:
        assert abs(done["tol"] - tol) <= 64 * kc.eps_of(torch.float64) * tol and done["rtol"] == rtol
    assert done["res"] <= done["tol"] < run.trace[k].st["res"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_iteration_limit_at_a_restart_boundary(dtype):
    """maxit = restart = 4: code 3 with column 4, the close applies, and begin(first=False) reports the limit (or
    convergence) without starting a cycle: V[0] keeps its bits."""
    n = 257
    run = _device_run("plain", n, dtype, 4)
    run.cycle(run.rhs, 4, 1e-30, 1e-50, 4, True)
    steps = [s for s in run.trace if s.what == "step"]
    assert [(s.st["stop"], s.st["kdone"]) for s in steps] == [(0, 1), (0, 2), (0, 3), (3, 4)]
    done = run.trace[-1].st
    assert (done["stop"], done["apply"], done["closed"], done["nt"], done["total"]) == (3, 1, 1, 4, 4)
    ref = kc.reference("plain", n, dtype, 12)
    true = float((ref.b - ref.A @ run.trace[-1].x.double()).norm())
    assert true <= ref.rho[4] + 64 * kc.eps_of(dtype) * ref.beta
    v0 = run.kr.V[0].clone()
    r = run.residual()
    vin = run.kr.vin.clone()
    run.ops.krylov_begin(run.kr, r, 0.0, 0.0, 0, False)
    s = run.snap("begin")
    assert s.st["stop"] == 3 and s.st["kdone"] == 0 and s.st["total"] == 4     # (1 only if x were converged: tol is 1e-30 beta)
    assert torch.equal(run.kr.V[0, :n], v0[:n]) and torch.equal(run.kr.vin[:n], vin[:n])     # (the pads were never written)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_right_hand_side_below_atol_is_solved_by_zero(dtype):
    n = 257
    run = _device_run("plain", n, dtype, 12)
    beta = float(run.rhs.double().norm())
    run.x.fill_(1.0)
    run.cycle(run.rhs, 2, 1e-30, 2.0 * beta, 10000, True)
    assert [(s.st["stop"], s.st["kdone"], s.st["total"]) for s in run.trace] == [(1, 0, 0)] * 4
    done = run.trace[-1].st
    assert done["apply"] == 0 and done["closed"] == 1 and done["res"] == done["beta"] and abs(done["beta"] - beta) <= 1e-6 * beta
    assert float(run.x.abs().max()) == 0.0
