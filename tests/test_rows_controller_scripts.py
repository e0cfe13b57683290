"""The scripts of tests/_ctl_scripts.py on the host form of the per-row controller (pn_rows_control_host, pn_rows_dense_plan_host):
no device.  These tests prove that the scripts reach the code they claim to reach -- every "at least one row takes this branch"
assertion is here -- and hold the host form to the invariants that need no reference.  tests/test_gpu_rows_controller.py then
holds pn_rows_control on the device to the host form, and to the same invariants."""
import pytest
import torch

import _ctl_scripts as cs
from pnode_amd._lib import PN_ROWS_FINISHED, PN_ROWS_H, PN_ROWS_REJ, PN_ROWS_STEPS

FORM_A = [("5dp", B) for B in cs.BATCHES] + [(rk, B) for rk in ("3bs", "5f", "2a") for B in (257, 8193)]


def test_the_tableaus_are_what_the_scripts_take_them_for():
    """5dp and 3bs are first-same-as-last, 5f and 2a are not.  The c of the last stage is a row sum of A in floating point: 1 for
    3bs, and one unit in the last place below 1 for 5dp -- the first-stage time of a 5dp row is t0 + c_last h0, which is not always
    the row's new time."""
    assert cs.tableau_end("3bs") == (True, 1.0)
    assert cs.tableau_end("5dp") == (True, 1.0 - 2.0 ** -52)
    assert not cs.tableau_end("5f")[0] and not cs.tableau_end("2a")[0]


def test_the_exact_norms_are_the_three_values_and_never_reject_for_long():
    B = 4096
    run = torch.zeros(B, dtype=torch.int64)
    worst, seen, rejecting = 0, set(), 0
    for k in range(cs.ROUND_CAP):
        e = cs.exact_norms(B, k)
        seen |= set(e.unique().tolist())
        run = torch.where(e > 1.0, run + 1, torch.zeros_like(run))
        worst = max(worst, int(run.max()))
        rejecting += int((e > 1.0).sum())
    assert seen == {0.0, 1e-30, 1e30}
    assert 3 <= worst <= cs.EXACT_REJECT_RUN < cs.MAX_REJECT
    assert 0.15 < rejecting / (B * cs.ROUND_CAP) < 0.25
    assert torch.equal(cs.exact_norms(B, 17), cs.exact_norms(B, 17)) and torch.equal(cs.exact_norms(B, 17)[:100], cs.exact_norms(100, 17))
    h0 = cs.exact_h0(B)
    assert set(h0.unique().tolist()) == {2.0 ** -k for k in range(4, 9)}
    assert float(h0.max()) <= float(cs.EXACT_SPAN[1])                      # no first step passes the first output time


@pytest.mark.parametrize("rk,B", FORM_A)
def test_exact_script_with_output_times_on_the_host(rk, B):
    ts = cs.make_ts(rk, **cs.EXACT_OPTIONS)
    inv = cs.SpanInvariants(B, cs.EXACT_SPAN, rk, exact=True)
    try:
        for pre, enorm, post in cs.host_rounds(ts, B, cs.EXACT_SPAN.numel(), cs.EXACT_SPAN, cs.EXACT_TMAX, cs.exact_h0(B), cs.exact_norms):
            # the premise of bit equality: no time or step the controller stores has rounded.  (The first-stage time of a 5dp
            # row is the one stored number that does round: its c_last is not 1.  SpanInvariants holds it to two roundings.)
            assert cs.is_dyadic(post.sd[cs.NOT_TFIRST]) and cs.is_dyadic(post.log_d[:2])
            inv.see(pre, post)
        inv.finish(post)
    finally:
        cs.free_ts(ts)
    assert inv.max_reject_run <= cs.EXACT_REJECT_RUN                           # no row came near ts_max_reject
    assert int(post.si[PN_ROWS_REJ].max()) > 0 and inv.rounds < 200
    print("%s, B = %d: %d rounds; steps cut %d, halved %d, stretched %d towards an output time; %d landings emptied the cache"
          % (rk, B, inv.rounds, inv.cuts, inv.halvings, inv.stretches, inv.cache_reset))
    if B > 1:
        assert inv.cuts > 0 and inv.halvings > 0 and inv.stretches > 0 and inv.cache_reset > 0
        assert max(inv.span_counters) > 1                                      # rows on different span counters in one launch
        assert len(inv.finish_rounds) > 1                                      # rows finishing in different rounds
        assert int(post.si[PN_ROWS_STEPS].max()) > int(post.si[PN_ROWS_STEPS].min())


@pytest.mark.parametrize("rk,B", [("5dp", 257), ("2a", 257)])
def test_fixed_step_script_brings_the_cached_step_back(rk, B):
    """With norm-driven steps the controller always chooses a new step at a landing (the factor is exactly 2, or the clamp), so
    `dt_span_cached` is only emptied there.  Without an error estimate the step stays, and the step cached before the approach
    comes back after the landing: that path, on the same output times."""
    ts = cs.make_ts(rk, **cs.EXACT_OPTIONS)
    inv = cs.SpanInvariants(B, cs.EXACT_SPAN, rk, exact=True, fixed=True)
    try:
        for pre, enorm, post in cs.host_rounds(ts, B, cs.EXACT_SPAN.numel(), cs.EXACT_SPAN, cs.EXACT_TMAX, cs.exact_h0(B, lo=6), cs.fixed_norms):
            assert cs.is_dyadic(post.sd[cs.NOT_TFIRST])
            inv.see(pre, post)
        inv.finish(post)
    finally:
        cs.free_ts(ts)
    assert inv.cache_back > 0 and inv.cuts > 0 and int(post.si[PN_ROWS_REJ].max()) == 0


@pytest.mark.parametrize("B", cs.BATCHES)
def test_exact_script_with_the_dense_plan_on_the_host(B):
    ts = cs.make_ts("5dp", **cs.EXACT_OPTIONS)
    inv = cs.DenseInvariants(B, cs.EXACT_DENSE_TIMES)
    rounds = 0
    try:
        for pre, enorm, post in cs.host_rounds(ts, B, 0, None, cs.EXACT_TMAX, cs.exact_h0(B), cs.exact_norms, dense_times=cs.EXACT_DENSE_TIMES):
            assert cs.is_dyadic(post.sd[cs.NOT_TFIRST])
            inv.see(pre, post)
            rounds += 1
        inv.finish(post)
    finally:
        cs.free_ts(ts)
    assert bool((post.si[PN_ROWS_FINISHED] == 1).all()) and rounds < 200
    assert inv.landings > 0                                                    # times[o] == tnew on an interior output


@pytest.mark.parametrize("name", sorted(cs.POW_OPTIONS))
def test_pow_scripts_take_their_branches(name):
    opts = cs.POW_OPTIONS[name]
    B = cs.POW_B
    ts = cs.make_ts("5dp", **opts)
    inv = cs.SpanInvariants(B, cs.POW_SPAN, "5dp")
    try:
        rounds = list(cs.host_rounds(ts, B, cs.POW_SPAN.numel(), cs.POW_SPAN, cs.POW_TMAX, cs.pow_h0(B), cs.pow_norms))
    finally:
        cs.free_ts(ts)
    for pre, enorm, post in rounds:
        inv.see(pre, post)
    forced, capped, again = cs.pow_branches(rounds, opts)
    print("%s: %d rounds; accepted above 1: %d, clamped to dt_max: %d, rejected after a rejection: %d" % (name, len(rounds), forced, capped, again))
    assert again > 0                                                           # reject_safety is in the factor
    assert (forced > 0) == (name == "dt_min")
    assert (capped > 0) == (name == "dt_max")
    assert len(inv.finish_rounds) > 1 and max(inv.span_counters) > 1
    assert float(cs.pow_h0(B).max()) <= float(cs.POW_SPAN[1])


@pytest.mark.parametrize("B", [1, 257, 8193])
def test_prepared_rounds_against_the_python_expectations(B):
    """The expectations the device test uses, checked against the host form first."""
    base, base_enorm = cs.summary_base(B)
    for max_steps in (None, cs.SUMMARY_STEPS + 1):
        ts = cs.make_ts("5dp") if max_steps is None else cs.make_ts("5dp", ts_max_steps=max_steps)
        try:
            for name, fails in cs.summary_cases(B) if max_steps is None else cs.summary_cases(B)[:1] + cs.summary_cases(B)[-1:]:
                pre, enorm = cs.summary_case(base, base_enorm, fails)
                post = cs.copy_state(pre)
                cs.control_host(ts, post, 0, None, cs.SUMMARY_TMAX, enorm)
                cs.check_summary_round(pre, enorm, post, fails, max_steps)
        finally:
            cs.free_ts(ts)
    if B > 1:
        done = int((base.si[PN_ROWS_FINISHED] != 0).sum())
        assert 0.25 * B < done < 0.42 * B and bool((base.sd[PN_ROWS_H][base.si[PN_ROWS_FINISHED] != 0] == 0).all())
        assert int((base_enorm > 1.0).sum()) > 0.1 * B
