"""-m gpu: pn_rows_control (csrc/pn_rows.hip) driven through whole solves against the host form of the same text
(pn_rows_control_host), with the scripts of tests/_ctl_scripts.py; tests/test_rows_controller_scripts.py proves on the host that
the scripts reach the branches they are written for.

  1. exact scripts: nothing the controller stores rounds, so every array of every round is the host's, bit for bit -- with the
     output times seen by the controller (form A, four tableaus) and with the dense plan carried from round to round (form B,
     pn_rows_dense_eval against pn_rows_dense_plan_host);
  2. scripts with pow in play: every round from the host's own input state; integers exactly, doubles to the 1e-14 that
     tests/test_gpu_sample_adapt.py grants the comparison of the two controllers (device pow against libm's);
  3. one prepared round with failing rows at the seams of the reduction: the summary against numbers computed from the inputs.

The batch sizes are chosen by the number of workgroups (256 rows each): 1, 2, 31 / 32 / 33 around the 32 shards of the arrival
counter, and 257 and 274, where the last workgroup reads the partials in two trips.  After every launch the arrival counters at
the start of the work area are zero again."""
import ctypes
import time

import pytest
import torch

import _ctl_scripts as cs
from conftest import require_gpu
from pnode_amd import _lib
from pnode_amd._lib import PN_ROWS_FINISHED, PN_ROWS_T

pytestmark = pytest.mark.gpu

FORM_A = [("5dp", B) for B in cs.BATCHES] + [(rk, B) for rk in ("3bs", "5f", "2a") for B in (257, 8193)]
D = 4                                               # the state of a form B row


def _ops(n):
    from pnode_amd.petsc_adjoint import HipVecOps
    return HipVecOps(require_gpu(), torch.float64, n)


def _ticket_clean(work):
    return not bool(work[:cs.NTICKET].view(torch.int64).any())


def _same_bits(got, want, names, where):
    for name in names:
        a, b = getattr(got, name), getattr(want, name)
        assert torch.equal(a, b), "%s: %s differs in %d entries" % (where, name, int((a != b).sum()))


def _lockstep(rk, B, norms, h0, inv, nspan, span, dense_times=None):
    """The host form and the device side by side, each on its own state, compared after every round; the invariants on the
    device's arrays.  Returns the device's last state."""
    ops = _ops(B * D)
    dev = ops.device
    ts = cs.make_ts(rk, **cs.EXACT_OPTIONS)
    work = cs.work_area(ops, B)
    start = cs.new_state(B, h0, nspan)
    names = cs.ARRAYS
    if dense_times is not None:
        cs.add_dense(start)
        names = cs.ARRAYS + ("next", "range")
        _, P = _lib.get_tableau_dense(rk)
        cols = [j for j in range(_lib.PN_MAX_STAGES) if any(v != 0.0 for v in P[j])]
        pv = [v for j in cols for v in list(P[j]) + [0.0] * (_lib.PN_DENSE_MAX_POW - len(P[j]))]
        Pc = (ctypes.c_double * len(pv))(*pv)
        nout = dense_times.numel()
        times_d = dense_times.to(dev)
        u, unew = torch.zeros(B * D, dtype=torch.float64, device=dev), torch.ones(B * D, dtype=torch.float64, device=dev)
        Ks = [torch.zeros(B * D, dtype=torch.float64, device=dev) for _ in cols]
        sol = torch.full((nout, B * D), float("nan"), dtype=torch.float64, device=dev)
    dst = cs.copy_state(start, dev)
    span_d = None if span is None else span.to(dev)
    mine = start
    try:
        for k, (pre, enorm, post) in enumerate(cs.host_rounds(ts, B, nspan, span, cs.EXACT_TMAX, h0, norms, dense_times=dense_times)):
            cs.control_device(ops, ts, dst, nspan, span_d, cs.EXACT_TMAX, enorm.to(dev), work)
            if dense_times is not None:
                ops.rows_dense_eval(B, D, sol, times_d, u, Ks, Pc, unew, dst.log_d, dst.sd[PN_ROWS_T], dst.log_hit, dst.next, dst.range)
            got = cs.copy_state(dst, "cpu")
            _same_bits(got, post, names, "round %d" % k)
            assert _ticket_clean(work), "round %d: an arrival counter was left non-zero" % k
            inv.see(mine, got)
            mine = got
        inv.finish(mine)
    finally:
        cs.free_ts(ts)
    if dense_times is not None:
        # every output but the first (the caller's initial state) has been written for every row; the last one is a copy
        assert bool(torch.isnan(sol[0]).all()) and not bool(torch.isnan(sol[1:]).any())
        assert bool((sol[nout - 1] == 1.0).all())
    return mine, k + 1


# ---------------------------------------------------------------------------------------------------------------- 1. exact scripts
@pytest.mark.parametrize("rk,B", FORM_A)
def test_exact_script_with_output_times(rk, B):
    inv = cs.SpanInvariants(B, cs.EXACT_SPAN, rk, exact=True)
    t0 = time.time()
    last, rounds = _lockstep(rk, B, cs.exact_norms, cs.exact_h0(B), inv, cs.EXACT_SPAN.numel(), cs.EXACT_SPAN)
    print("%s, B = %d: %d rounds in %.2f s, bit for bit" % (rk, B, rounds, time.time() - t0))
    assert inv.max_reject_run <= cs.EXACT_REJECT_RUN and rounds < 200
    if B > 1:
        assert inv.cuts > 0 and inv.halvings > 0 and inv.stretches > 0 and inv.cache_reset > 0
        assert max(inv.span_counters) > 1 and len(inv.finish_rounds) > 1


@pytest.mark.parametrize("rk,B", [("5dp", 257), ("2a", 257)])
def test_fixed_step_script_brings_the_cached_step_back(rk, B):
    inv = cs.SpanInvariants(B, cs.EXACT_SPAN, rk, exact=True, fixed=True)
    _lockstep(rk, B, cs.fixed_norms, cs.exact_h0(B, lo=6), inv, cs.EXACT_SPAN.numel(), cs.EXACT_SPAN)
    assert inv.cache_back > 0 and inv.cuts > 0


@pytest.mark.parametrize("B", cs.BATCHES)
def test_exact_script_with_the_dense_plan(B):
    inv = cs.DenseInvariants(B, cs.EXACT_DENSE_TIMES)
    t0 = time.time()
    last, rounds = _lockstep("5dp", B, cs.exact_norms, cs.exact_h0(B), inv, 0, None, dense_times=cs.EXACT_DENSE_TIMES)
    print("dense plan, B = %d: %d rounds in %.2f s, bit for bit; %d landings on an interior output" % (B, rounds, time.time() - t0, inv.landings))
    assert bool((last.si[PN_ROWS_FINISHED] == 1).all()) and rounds < 200
    assert inv.landings > 0


# ---------------------------------------------------------------------------------------------------------------- 2. pow in play
@pytest.mark.parametrize("name", sorted(cs.POW_OPTIONS))
def test_pow_scripts_round_by_round_from_the_hosts_state(name):
    """Nothing compounds: every device round starts from the host's bits."""
    opts = cs.POW_OPTIONS[name]
    B, nspan = cs.POW_B, cs.POW_SPAN.numel()
    ops = _ops(B)
    dev = ops.device
    ts = cs.make_ts("5dp", **opts)
    span_d = cs.POW_SPAN.to(dev)
    off = 0
    try:
        rounds = list(cs.host_rounds(ts, B, nspan, cs.POW_SPAN, cs.POW_TMAX, cs.pow_h0(B), cs.pow_norms))
        forced, capped, again = cs.pow_branches(rounds, opts)
        assert again > 0 and (forced > 0) == (name == "dt_min") and (capped > 0) == (name == "dt_max")
        for k, (pre, enorm, post) in enumerate(rounds):
            dst = cs.copy_state(pre, dev)
            ops.rows_control(ts, B, nspan, span_d, cs.POW_TMAX, enorm.to(dev), dst.sd, dst.si, dst.log_d, dst.log_hit, dst.accept, dst.summary)
            got = cs.copy_state(dst, "cpu")
            off += int((got.sd != post.sd).sum()) + int((got.log_d != post.log_d).sum())
            _same_bits(got, post, ("si", "log_hit", "accept", "summary"), "round %d" % k)
            for nm in ("sd", "log_d"):
                assert torch.allclose(getattr(got, nm), getattr(post, nm), rtol=1e-14, atol=0.0), (k, nm)
    finally:
        cs.free_ts(ts)
    print("%s: %d rounds of %d rows; doubles that are not the host's bits: %d" % (name, len(rounds), B, off))


# ---------------------------------------------------------------------------------------------------------------- 3. the summary
@pytest.mark.parametrize("B", cs.SUMMARY_BATCHES)
def test_summary_and_failure_codes(B):
    ops = _ops(B)
    dev = ops.device
    work = cs.work_area(ops, B)
    base, base_enorm = cs.summary_base(B)
    ncase = 0
    for max_steps in (None, cs.SUMMARY_STEPS + 1):
        ts = cs.make_ts("5dp") if max_steps is None else cs.make_ts("5dp", ts_max_steps=max_steps)
        cases = cs.summary_cases(B)
        try:
            for name, fails in cases if max_steps is None else cases[:1] + cases[-1:]:
                pre, enorm = cs.summary_case(base, base_enorm, fails)
                pre_d, enorm_d = cs.copy_state(pre, dev), enorm.to(dev)
                first = None
                for launch in range(3):                    # the same work area, launch after launch
                    dst = cs.copy_state(pre_d)
                    cs.control_device(ops, ts, dst, 0, None, cs.SUMMARY_TMAX, enorm_d, work)
                    assert _ticket_clean(work), (name, launch)
                    if first is None:
                        first = dst
                    else:
                        _same_bits(dst, first, cs.ARRAYS, "%s, launch %d" % (name, launch))
                got = cs.copy_state(first, "cpu")
                cs.check_summary_round(pre, enorm, got, fails, max_steps)
                host = cs.copy_state(pre)
                cs.control_host(ts, host, 0, None, cs.SUMMARY_TMAX, enorm)
                _same_bits(got, host, ("si", "log_hit", "accept", "summary"), name)
                for nm in ("sd", "log_d"):
                    assert torch.allclose(getattr(got, nm), getattr(host, nm), rtol=1e-14, atol=0.0), (name, nm)
                ncase += 1
        finally:
            cs.free_ts(ts)
    assert ncase >= 5
