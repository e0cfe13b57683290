"""-pn_rows_compact 0|1 on the CPU stand-in (tests/_cpu_rows_compact_ops.py), fp64: func is evaluated and
differentiated on the rows of a round that have work to do, and nothing else changes.

With a func that is row-independent to the bit (the spirals of tests/_rows_compact_cases.py) 1 reproduces 0 exactly: the solution,
both gradients and every row's step log.  RateMLP's Linear layers run through the library GEMM, whose rounding may depend on the
number of rows it is given: there the counts (steps, rejections, rounds) are equal and the solution and the gradients agree within
1e-12 relative -- the bound the per-sample tests use against autograd (tests/test_sample_adapt.py).  Its step LOG cannot be held
to that: the controller turns round-off into step size.  The error estimate is a difference of size tol * |u| between two
solutions of size |u|, so a relative perturbation eps = 2^-52 of the stage derivatives moves the error norm by up to eps / tol
relative, and the next step size h * safety * enorm^(-1/order) with it; every step inherits its predecessor's h.  The n-th logged
step size of a row is therefore compared within n * eps / tol relative (measured on this MLP: about 1e-10 at tol 1e-8), its time,
a sum of step sizes, within that fraction of the span.  The solution feels such a change of h only through the local error, of
size tol: eps again."""
import pytest
import torch

import _rows_compact_cases as C
from _cpu_rows_compact_ops import CpuRowsCompactOps, RowsCompactMixin
from _cpu_rows_tgrad_ops import CpuRowsTgradOps
from _winf_cases import CpuWinfOps
from pnode_amd import _lib, options, petsc_adjoint
from pnode_amd._lib import PnError

B = 8
STAGES = {"5dp": 7, "3bs": 4}                     # func evaluations of one forward round: every stage of the tableau


class CpuWinfCompactOps(RowsCompactMixin, CpuWinfOps):
    pass


# name -> (tableau, options, t.requires_grad, backend)
MODES = {
    "recomputed": ("5dp", (("ts_trajectory_solution_only", "1"),), False, CpuRowsCompactOps),
    "stored": ("5dp", (("ts_trajectory_solution_only", "0"),), False, CpuRowsCompactOps),
    "interp-3bs": ("3bs", (("pn_output_times", "interpolate"),), False, CpuRowsCompactOps),
    "interp-5dp": ("5dp", (("pn_output_times", "interpolate"),), False, CpuRowsCompactOps),
    "tgrad-match": ("5dp", (), True, CpuRowsCompactOps),
    "tgrad-interp": ("5dp", (("pn_output_times", "interpolate"),), True, CpuRowsCompactOps),
    "infinity": ("5dp", (("ts_adapt_wnormtype", "infinity"),), False, CpuWinfCompactOps),
}

_PAIRS = {}


def _pair(func, mode):
    """(the solve without compaction, the solve with it) of one func and mode: computed once, shared by the tests below."""
    if (func, mode) not in _PAIRS:
        rk, extra, tgrad, backend = MODES[mode]
        _PAIRS[(func, mode)] = tuple(C.solve(backend, c, func=func, B=B, rk=rk, extra=extra, tgrad=tgrad) for c in ("0", "1"))
    return _PAIRS[(func, mode)]


def _same_counts(a, b):
    oa, ob = a["ode"], b["ode"]
    assert torch.equal(oa.sample_steps, ob.sample_steps) and torch.equal(oa.sample_rejections, ob.sample_rejections)
    assert oa.rounds == ob.rounds and oa.nfe_forward == ob.nfe_forward


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_row_independent_func_gives_the_same_bits(mode):
    off, on = _pair("spiral", mode)
    _same_counts(off, on)
    assert off["logs"] == on["logs"]
    assert int(off["ode"].sample_steps.min()) * 2 <= int(off["ode"].sample_steps.max())
    for key in ("sol", "gu", "gp"):
        assert torch.equal(off[key], on[key]), key
    if MODES[mode][2]:
        assert float(off["gt"].abs().min()) > 0.0
        assert C.rel(on["gt"], off["gt"]) <= 1e-12 and C.rel(on["dtrow"], off["dtrow"]) <= 1e-12
    assert on["ode"].rows_evaluated < off["ode"].rows_evaluated


# (the time-dependent spiral: <w, df/dt> per row travels through the scatter; its drift's gradient is a sum over the rows func was
# given, which rounds with their number -- round-off, not bits)
@pytest.mark.parametrize("func,mode", [("mlp", m) for m in sorted(MODES)] + [("time", "tgrad-match"), ("time", "tgrad-interp")])
def test_an_mlp_on_a_spread_batch_agrees_to_round_off(func, mode):
    off, on = _pair(func, mode)
    steps = off["ode"].sample_steps
    assert int(steps.min()) <= int(steps.max()) / 2, steps           # the uncompacted solve itself: the rows' step counts are spread
    _same_counts(off, on)
    tol = C.TOL[MODES[mode][0]]
    for la, lb in zip(off["logs"], on["logs"]):
        assert len(la) == len(lb)
        for n, ((ta, ha), (tb, hb)) in enumerate(zip(la, lb)):
            bound = (n + 1) * 2.0 ** -52 / tol                     # (the module's docstring)
            assert abs(ha - hb) <= bound * ha and abs(ta - tb) <= bound * C.TIMES[-1], (n, ta, tb, ha, hb)
    worst = {key: C.rel(on[key], off[key]) for key in ("sol", "gu", "gp")}
    if MODES[mode][2]:
        worst["gt"], worst["dtrow"] = C.rel(on["gt"], off["gt"]), C.rel(on["dtrow"], off["dtrow"])
    print("%s %s: steps %s, 1 against 0 %s" % (func, mode, steps.tolist(), worst))
    assert max(worst.values()) <= 1e-12, worst
    assert on["ode"].rows_evaluated < 0.75 * off["ode"].rows_evaluated


def _heff(ode):
    return torch.stack([ode._round_log[k].heff for k in range(ode.rounds)]) > 0.0          # [rounds][B]


@pytest.mark.parametrize("func,mode", [("mlp", m) for m in sorted(MODES)] + [("spiral", "recomputed"), ("time", "tgrad-interp")])
def test_the_counters_are_the_work_the_round_log_shows(func, mode):
    off, on = _pair(func, mode)
    o0, o1 = off["ode"], on["ode"]
    assert o0.rows_compact == "off"
    assert o0.rows_evaluated == B * o0.nfe_forward and o0.rows_evaluated_backward == B * o0.nfe_backward
    moved = _heff(o0)
    # a row finishes with an accepted step: it is open at the start of round k iff it moves in round k or later
    last = torch.tensor([int(moved[:, r].nonzero().max()) for r in range(B)])
    nopen = [int((last >= k).sum()) for k in range(o0.rounds)]
    assert nopen[0] == B and nopen[-1] >= 1
    assert o1.rows_evaluated == sum(nopen) * STAGES[MODES[mode][0]]
    per_round = o0.nfe_backward // o0.rounds                        # stage evaluations of a reversed round
    assert per_round * o0.rounds == o0.nfe_backward
    assert o1.rows_evaluated_backward == int(moved.sum()) * per_round
    assert o1.nfe_backward == per_round * int(moved.any(1).sum())
    assert o1.rows_compact == "on (rows evaluated %d of %d forward, %d of %d backward)" % (
        o1.rows_evaluated, o0.rows_evaluated, o1.rows_evaluated_backward, o0.rows_evaluated_backward)


def test_a_reversed_round_in_which_no_row_moved_is_crossed():
    kw = dict(func="spiral", B=1, step_size=0.2, times=[0.0, 0.2])
    off, on = (C.solve(CpuRowsCompactOps, c, **kw) for c in ("0", "1"))
    assert int(off["ode"].sample_rejections[0]) >= 1                # the first step is far too long: a round of its own, h_eff = 0
    _same_counts(off, on)
    assert not bool(_heff(on["ode"]).all())
    assert on["ode"].nfe_backward < off["ode"].nfe_backward and on["ode"].rows_evaluated == off["ode"].rows_evaluated
    for key in ("sol", "gu", "gp"):
        assert torch.equal(off[key], on[key]), key
    # and with dL/dt and interpolated outputs, whose bookkeeping runs in that round too
    kw = dict(func="time", B=1, step_size=0.2, tgrad=True, extra=(("pn_output_times", "interpolate"),))
    off, on = (C.solve(CpuRowsCompactOps, c, **kw) for c in ("0", "1"))
    assert int(off["ode"].sample_rejections[0]) >= 1
    for key in ("sol", "gu", "gp"):
        assert torch.equal(off[key], on[key]), key
    assert C.rel(on["gt"], off["gt"]) <= 1e-12 and C.rel(on["dtrow"], off["dtrow"]) <= 1e-12


def test_func_sees_fewer_rows_as_the_rounds_go_by():
    shapes = {}
    for c in ("0", "1"):
        f = C.Recording()
        out = C.solve(CpuRowsCompactOps, c, func="spiral", B=B, module=f)
        n = out["ode"].nfe_forward
        shapes[c] = f.shapes
        assert len(f.shapes) == n + out["ode"].nfe_backward
        for ys, ts in f.shapes:
            assert ys[1:] == (2,) and ts == (ys[0], 1)
    assert all(ys[0] == B for ys, _ in shapes["0"])
    fwd = [ys[0] for ys, _ in shapes["1"][:n]]
    assert fwd[0] == B and fwd[-1] < B and all(a >= b for a, b in zip(fwd, fwd[1:])) and len(set(fwd)) >= 3
    assert all(1 <= ys[0] <= B for ys, _ in shapes["1"][n:]) and min(ys[0] for ys, _ in shapes["1"][n:]) < B


def test_refusals():
    y = C.spiral_y0(4)

    def setup(backend, **opts):
        options.clear()
        for k, v in opts.items():
            options.set_option(k, v)
        ode = petsc_adjoint.ODEPetsc(backend=backend)
        ode.setupTS(y, C.SpiralTruth(), step_size=0.01, method="dopri5", enable_adjoint=True)
        return ode

    with pytest.raises(PnError, match="-pn_rows_compact 1 needs -pn_adapt_scope sample"):
        setup(CpuRowsCompactOps, pn_adapt_scope="batch", pn_rows_compact="1")
    with pytest.raises(PnError, match="-pn_rows_compact 1 needs -pn_adapt_scope sample"):
        setup(CpuRowsCompactOps, pn_rows_compact="1")
    with pytest.raises(PnError, match="-pn_rows_compact 1 is not built on this backend"):
        setup(CpuRowsTgradOps, pn_adapt_scope="sample", pn_rows_compact="1")
    for bad in ("2", "on", "-1", ""):
        with pytest.raises(PnError, match="-pn_rows_compact must be 0 or 1"):
            setup(CpuRowsCompactOps, pn_adapt_scope="sample", pn_rows_compact=bad)
    assert setup(CpuRowsTgradOps, pn_adapt_scope="sample", pn_rows_compact="0").rows_compact == "off"
    assert setup(CpuRowsCompactOps, pn_adapt_scope="batch", pn_rows_compact="0").rows_compact == "off"
    assert setup(CpuRowsCompactOps, pn_adapt_scope="sample", pn_rows_compact="1").rows_compact.startswith("on (rows evaluated 0 of 0")


def test_ts_view_reports_the_ratios(capsys):
    C.solve(CpuRowsCompactOps, "1", func="spiral", B=B, extra=(("ts_view", ""),))
    line = [l for l in capsys.readouterr().out.splitlines() if "-pn_adapt_scope sample" in l and "rounds for" in l]
    assert line and "-pn_rows_compact: on (rows evaluated " in line[0]
    C.solve(CpuRowsCompactOps, "0", func="spiral", B=B, extra=(("ts_view", ""),))
    assert "pn_rows_compact" not in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- pn_rows_list_host
def list_patterns(n):
    """name -> which of n rows are listed"""
    pats = {"all": [True] * n, "none": [False] * n, "alternating": [r % 2 == 0 for r in range(n)], "last": [r == n - 1 for r in range(n)]}
    g = torch.Generator().manual_seed(n)
    pats["random"] = (torch.rand(n, generator=g) < 0.3).tolist()
    return pats


def list_source(kind, listed, nan_at=None):
    """The source vector of pn_rows_list with `listed` rows listed: kind 0 the int32 finished codes, kind 1 fp64 h_eff (an unlisted
    row is 0, -0.0 or negative in turn; `nan_at`: that row holds a NaN, which is not listed)."""
    n = len(listed)
    if kind == 0:
        return torch.tensor([0 if on else 1 + r % 3 for r, on in enumerate(listed)], dtype=torch.int32)
    src = torch.tensor([0.125 * (1 + r % 5) if on else (0.0, -0.0, -1.0)[r % 3] for r, on in enumerate(listed)], dtype=torch.float64)
    if nan_at is not None:
        src[nan_at] = float("nan")
    return src


def check_list(listed, idx, pos, count):
    n = len(listed)
    want = [r for r in range(n) if listed[r]]
    m = len(want)
    assert count.tolist() == [m]
    assert idx.tolist() == want + [-1] * (n - m)                                     # ascending, then the -1 tail
    inv = [-1] * n
    for k, r in enumerate(want):
        inv[r] = k
    assert pos.tolist() == inv


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 9, 64, 257])
def test_rows_list_host(kind, n):
    lib = _lib.load()
    cases = list(list_patterns(n).items())
    if kind == 1:
        cases.append(("nan", [r != n // 2 for r in range(n)]))
    for name, listed in cases:
        src = list_source(kind, listed, nan_at=n // 2 if name == "nan" else None)
        idx, pos, count = (torch.full((k,), 77, dtype=torch.int32) for k in (n, n, 1))
        _lib.check(lib.pn_rows_list_host(n, kind, src.data_ptr(), idx.data_ptr(), pos.data_ptr(), count.data_ptr()))
        check_list(listed, idx, pos, count)
    one = torch.zeros(1, dtype=torch.int32)
    assert lib.pn_rows_list_host(0, 0, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr()) != 0
    assert lib.pn_rows_list_host(1, 2, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr()) != 0
    assert b"pn_rows_list_host" in lib.pn_last_error()
    assert lib.pn_rows_list(None, 1, 0, None, one.data_ptr(), one.data_ptr(), one.data_ptr(), None) != 0      # refused before any launch
    assert lib.pn_rows_gather(None, 7, 1, 1, one.data_ptr(), one.data_ptr(), one.data_ptr()) != 0
    assert lib.pn_last_error() == b"pn_rows_gather: unknown dtype"
    assert lib.pn_rows_scatter(None, 7, 1, 1, one.data_ptr(), one.data_ptr(), one.data_ptr()) != 0
    assert lib.pn_last_error() == b"pn_rows_scatter: unknown dtype"
    assert lib.pn_rows_gather(None, _lib.PN_F64, 0, 4, None, None, None) == 0                                   # nothing to gather
