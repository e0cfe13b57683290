"""TEST SCAFFOLDING -- scripted solves for the per-row step controller (pn_ctl_judge / pn_rows_judge_row, csrc/pn_adapt.h), shared
by tests/test_rows_controller_scripts.py (the host form, no device) and tests/test_gpu_rows_controller.py (pn_rows_control on the
device against the host form).  A script fixes every row's first step, the output times and the error norm of row r in round k; the
norm does not depend on the step, so the controller is driven through whole solves without any state vector.

Three families:
  * exact scripts: every time and step is a dyadic number with few bits and the step factor is clipped to exactly 2 or 0.5, so no
    operation whose result is stored rounds -- host and device must agree in every bit (`exact_*`);
  * scripts with pow in play: lognormal norms, steps and output times that are no dyadic numbers (`pow_*`);
  * one prepared round with failing rows at chosen positions (`summary_case`).
The invariant classes check what needs no reference; they take arrays on the host (the device test copies its arrays over)."""
import ctypes
import types

import torch

from pnode_amd import _lib
from pnode_amd._lib import (PN_ROWS_CACHED, PN_ROWS_FAIL, PN_ROWS_FINISHED, PN_ROWS_H, PN_ROWS_ND, PN_ROWS_NI, PN_ROWS_PREV_REJ,
                            PN_ROWS_REJ, PN_ROWS_REJ_STEP, PN_ROWS_SPANCTR, PN_ROWS_STEPS, PN_ROWS_T, PN_ROWS_TFIRST)

WG = 256                                             # rows per workgroup of pn_rows_control (kBlock)
WAVE = 64
NTICKET = 33 * 16                                    # (kTicketShards + 1) * kTicketStride doubles (csrc/pn_device.h)
# by the number of workgroups: 1, 2, either side of the 32 ticket shards, and 257 (the last workgroup's strided read of the
# partials takes a second trip)
BATCHES = [1, 257, 31 * WG, 32 * WG, 32 * WG + 1, 256 * WG + 1]
ROUND_CAP = 400                                      # asserted, never looped on: the exact scripts need well under 200 rounds
MAX_REJECT = 10                                      # the controller's default ts_max_reject


# ---------------------------------------------------------------------------------------------------------------- plumbing
def make_ts(rk, **options):
    """A pn_ts handle with the tableau `rk` and the given controller options (pn_ts_set_option); free it with free_ts."""
    lib = _lib.load()
    ts = ctypes.c_void_p(lib.pn_ts_create())
    _lib.check(lib.pn_ts_set_rk_type(ts, rk.encode()))
    for k, v in options.items():
        _lib.check(lib.pn_ts_set_option(ts, k.encode(), (v if isinstance(v, str) else repr(v)).encode()))
    return ts


def free_ts(ts):
    _lib.load().pn_ts_destroy(ts)


def tableau_end(rk):
    """(first-same-as-last?, c of the last stage) as rows_ctl_config hands them to the controller."""
    t = _lib.get_tableau(rk)
    return bool(t.fsal), float(t.c[t.s - 1])


def new_state(B, h0, nspan, t0=0.0):
    """The arrays of a solve at its start, on the host: every row at t0 with its own first step, output 0 served."""
    st = types.SimpleNamespace(B=B)
    st.sd = torch.zeros(PN_ROWS_ND, B, dtype=torch.float64)
    st.sd[PN_ROWS_T] = t0
    st.sd[PN_ROWS_H] = h0
    st.sd[PN_ROWS_TFIRST] = st.sd[PN_ROWS_T]
    st.si = torch.zeros(PN_ROWS_NI, B, dtype=torch.int32)
    if nspan:
        st.si[PN_ROWS_SPANCTR] = 1
    fresh_outputs(st)
    return st


def fresh_outputs(st):
    """What a round writes, pre-filled with a value no round writes."""
    B = st.B
    st.log_d = torch.full((3, B), -7.0, dtype=torch.float64)
    st.log_hit = torch.full((B,), -7, dtype=torch.int32)
    st.accept = torch.full((B,), -7, dtype=torch.int32)
    st.summary = torch.full((4,), -7, dtype=torch.int32)


ARRAYS = ("sd", "si", "log_d", "log_hit", "accept", "summary")


def copy_state(st, dev=None):
    out = types.SimpleNamespace(B=st.B)
    for k in ARRAYS + tuple(k for k in ("next", "range") if hasattr(st, k)):
        v = getattr(st, k)
        setattr(out, k, v.clone() if dev is None else v.to(dev, copy=True))
    return out


def control_host(ts, st, nspan, span, tmax, enorm):
    _lib.check(_lib.load().pn_rows_control_host(ts, st.B, nspan, None if span is None else span.data_ptr(), tmax, enorm.data_ptr(),
                                                st.sd.data_ptr(), st.si.data_ptr(), st.log_d.data_ptr(), st.log_hit.data_ptr(),
                                                st.accept.data_ptr(), st.summary.data_ptr()))


def control_device(ops, ts, st, nspan, span, tmax, enorm, work):
    """pn_rows_control through the library itself, on a work area of the caller's (pn_rows_work_bytes(B), zero-filled once)."""
    _lib.check(ops.lib.pn_rows_control(ops.stream(), ts, st.B, nspan, None if span is None else span.data_ptr(), tmax,
                                       enorm.data_ptr(), st.sd.data_ptr(), st.si.data_ptr(), st.log_d.data_ptr(),
                                       st.log_hit.data_ptr(), st.accept.data_ptr(), st.summary.data_ptr(), work.data_ptr()))


def work_area(ops, B):
    return torch.zeros(ops.lib.pn_rows_work_bytes(B) // 8, dtype=torch.float64, device=ops.device)


def add_dense(st):
    """The rows' output counters of -pn_output_times interpolate: output 0 is the initial state itself."""
    st.next = torch.ones(st.B, dtype=torch.int32)
    st.range = torch.full((2, st.B), -7, dtype=torch.int32)


def dense_plan_host(st, times):
    """pn_rows_dense_eval's plan of the round st has just judged, on host arrays: log_hit becomes the output copied."""
    tnew = st.sd[PN_ROWS_T].contiguous()
    _lib.check(_lib.load().pn_rows_dense_plan_host(st.B, times.numel(), times.data_ptr(), st.log_d.data_ptr(), tnew.data_ptr(),
                                                   st.log_hit.data_ptr(), st.next.data_ptr(), st.range.data_ptr(), 0, None, None))


def host_rounds(ts, B, nspan, span, tmax, h0, norms, dense_times=None, cap=ROUND_CAP):
    """Drive the host form to completion.  Yields, per round k, (pre, enorm, post): the state the round started from, its
    error norms and the state it left (copies).  The cap is asserted."""
    st = new_state(B, h0, nspan)
    if dense_times is not None:
        add_dense(st)
    k = 0
    while True:
        assert k < cap, "the script did not finish in %d rounds" % cap
        pre = copy_state(st)
        enorm = norms(B, k)
        control_host(ts, st, nspan, span, tmax, enorm)
        if dense_times is not None:
            dense_plan_host(st, dense_times)
        yield pre, enorm, copy_state(st)
        if int(st.summary[0]) == 0:
            return
        k += 1


# ---------------------------------------------------------------------------------------------------------------- exact scripts
# in units of 2^-7: multiples of 2^-5 and three times (11, 37, 107) that are on no row's step grid.  The first one is not below the
# largest first step: the controller matches the step AFTER an accepted one, a solve's first step is clamped by its caller.
EXACT_SPAN = torch.tensor([0, 8, 11, 16, 20, 37, 64, 96, 107, 128], dtype=torch.float64) / 128.0
# the output times of the dense form (the controller sees none of them): dyadic ones, which rows land on, and others
EXACT_DENSE_TIMES = torch.tensor([0, 3, 8, 11, 16, 24, 37, 48, 64, 65, 96, 107, 120, 128], dtype=torch.float64) / 128.0
EXACT_TMAX = 1.0
EXACT_OPTIONS = dict(ts_adapt_clip="0.5,2", ts_adapt_dt_max=2.0 ** -4)
EXACT_REJECT_RUN = 5                                 # the longest run of rejecting norms a row can meet: below MAX_REJECT


def exact_h0(B, lo=8, hi=4):
    """2^-lo .. 2^-hi, varying by row."""
    r = torch.arange(B, dtype=torch.int64)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), -(hi + (r * 7 + r // 5) % (lo - hi + 1)).double())


def _hash(B, k):
    m = 0xFFFFFFFF
    x = (torch.arange(B, dtype=torch.int64) * 1540483477 + (k + 1) * 1274126177) & m
    x = x ^ (x >> 15)
    x = (x * 1274126177) & m
    x = x ^ (x >> 13)
    x = (x * 1540483477) & m
    return x ^ (x >> 16)


def exact_norms(B, k):
    """0.0 (factor infinite, clipped to 2), 1e-30 (factor far above the clip: 2) or 1e30 (rejected, factor clipped to 0.5) by
    a fixed hash of (row, round).  A quarter of the norms rejects, none in every sixth round: no row meets more than
    EXACT_REJECT_RUN rejections in a row, so none fails with ts_max_reject."""
    v = _hash(B, k) % 8
    e = torch.where(v < 5, torch.zeros(B, dtype=torch.float64), torch.full((B,), 1e-30, dtype=torch.float64))
    if k % (EXACT_REJECT_RUN + 1) != EXACT_REJECT_RUN:
        e = torch.where(v < 2, torch.full((B,), 1e30, dtype=torch.float64), e)
    return e


def fixed_norms(B, k):
    """No error estimate (a negative norm): every attempt is accepted with the step it had.  The one way to a step the
    controller has not chosen anew, which is what brings the cached step back after a landing."""
    return torch.full((B,), -1.0, dtype=torch.float64)


NOT_TFIRST = [PN_ROWS_T, PN_ROWS_H, PN_ROWS_CACHED]


def is_dyadic(x, bits=45):
    """Every entry is a multiple of 2^-bits (and below 2^(53 - bits)): sums and differences of such numbers do not round."""
    y = x * 2.0 ** bits
    return bool((y == y.round()).all()) and bool((x.abs() <= 2.0 ** (52 - bits)).all())


class SpanInvariants:
    """What holds for every round of a solve whose controller sees the output times, whatever the norms (form A)."""

    def __init__(self, B, span, rk, exact=False, fixed=False):
        self.B, self.span, self.exact, self.fixed = B, span, exact, fixed
        self.tmax = float(span[-1])
        self.fsal, self.c_last = tableau_end(rk)
        self.next_hit = torch.ones(B, dtype=torch.int64)
        self.accepted = torch.zeros(B, dtype=torch.int64)
        self.rejected = torch.zeros(B, dtype=torch.int64)
        self.cache_reset = self.cache_back = self.cuts = self.halvings = self.stretches = 0
        self.max_reject_run = 0
        self.span_counters = set()                   # how many different counters one launch has seen
        self.finish_rounds = set()
        self.rounds = 0

    def see(self, pre, post):
        sd0, si0, sd, si = pre.sd, pre.si, post.sd, post.si
        was_open = si0[PN_ROWS_FINISHED] == 0
        acc = post.accept == 1
        assert bool(((post.accept == 0) | acc).all()) and not bool((acc & ~was_open).any())
        # the round's log: the attempt's start, and the step where it was accepted
        assert torch.equal(post.log_d[1], sd0[PN_ROWS_T]) and torch.equal(post.log_d[2], sd0[PN_ROWS_TFIRST])
        assert torch.equal(post.log_d[0], torch.where(acc, sd0[PN_ROWS_H], torch.zeros_like(sd0[PN_ROWS_H])))
        # every output index once and in ascending order, the time at a hit that output time's bits
        hit = post.log_hit >= 0
        assert not bool((hit & ~acc).any()) and bool((post.log_hit[~hit] == -1).all())
        assert torch.equal(post.log_hit[hit].long(), self.next_hit[hit])
        assert torch.equal(sd[PN_ROWS_T][hit], self.span[post.log_hit[hit].long()])
        self.next_hit[hit] += 1
        assert torch.equal(si[PN_ROWS_SPANCTR].long(), self.next_hit)
        self.span_counters.add(int(si0[PN_ROWS_SPANCTR][was_open].unique().numel()))
        # time: a rejected or closed row stays; (exact scripts) an accepted one moves by its step, no rounding
        assert torch.equal(sd[PN_ROWS_T][~acc], sd0[PN_ROWS_T][~acc])
        if self.exact:
            assert torch.equal(sd[PN_ROWS_T][acc], (sd0[PN_ROWS_T] + sd0[PN_ROWS_H])[acc])
        # where the next first stage derivative is evaluated
        first = (sd0[PN_ROWS_T] + self.c_last * sd0[PN_ROWS_H]) if self.fsal else sd[PN_ROWS_T]
        assert torch.equal(sd[PN_ROWS_TFIRST], torch.where(acc, first, sd0[PN_ROWS_TFIRST]))
        # counters
        failed = si[PN_ROWS_FAIL] != 0
        self.accepted += acc
        self.rejected += was_open & ~acc & (si[PN_ROWS_FAIL] != 1)
        assert torch.equal(si[PN_ROWS_STEPS].long(), self.accepted) and torch.equal(si[PN_ROWS_REJ].long(), self.rejected)
        self.max_reject_run = max(self.max_reject_run, int(si[PN_ROWS_REJ_STEP].max()))
        # finished rows: h = 0 from the round that finishes them, and every later round is the identity on them
        fin = si[PN_ROWS_FINISHED] != 0
        assert bool((sd[PN_ROWS_H][fin] == 0.0).all()) and bool((sd[PN_ROWS_H][~fin] > 0.0).all())
        closed = ~was_open
        assert torch.equal(sd[:, closed], sd0[:, closed]) and torch.equal(si[:, closed], si0[:, closed])
        assert bool((post.log_d[0][closed] == 0.0).all()) and bool((post.log_hit[closed] == -1).all())
        assert bool((si[PN_ROWS_FINISHED][fin & was_open & ~failed & (sd[PN_ROWS_T] >= self.tmax)] == 1).all())
        if bool((fin & was_open).any()):
            self.finish_rounds.add(self.rounds)
        # the summary
        first_fail = int(failed.nonzero()[0]) if bool(failed.any()) else -1
        assert post.summary.tolist() == [int((~fin).sum()), first_fail, int(si[PN_ROWS_FAIL][first_fail]) if first_fail >= 0 else 0, 0]
        # the step cached when an approach to an output time was first adjusted: cut onto it, halved (two steps to it) or
        # stretched by up to match_stretch onto it.  At the landing the cache is emptied, and filled again only by an adjustment
        # towards the next time
        c0, c1, h1 = sd0[PN_ROWS_CACHED], sd[PN_ROWS_CACHED], sd[PN_ROWS_H]
        assert torch.equal(c1[~acc], c0[~acc])
        newly = acc & (c1 > 0) & ~fin & ((c0 == 0) | hit)
        assert bool((h1 != c1)[newly].all()) and bool((h1 <= 1.01 * c1)[newly].all())
        left = self.span[self.next_hit.clamp(max=self.span.numel() - 1)] - sd[PN_ROWS_T]          # (exact scripts: no rounding)
        self.cuts += int((newly & (h1 < c1) & (h1 == left)).sum())
        self.halvings += int((newly & (h1 < c1) & (2.0 * h1 == left)).sum())
        self.stretches += int((newly & (h1 > c1)).sum())
        if self.exact:
            assert bool(((h1 == left) | (2.0 * h1 == left))[newly].all())
        kept = acc & ~hit & (c0 > 0)
        assert torch.equal(c1[kept], c0[kept])
        land = hit & (c0 > 0) & ~fin
        self.cache_reset += int((land & (c1 == 0)).sum())
        if self.fixed:
            # the controller chose no new step: the cached one comes back, unless it is cut again at once (and then stays cached)
            back = land & (h1 == c0) & (c1 == 0)
            again = land & (c1 == c0) & (h1 < c0)
            assert bool((back | again)[land].all())
            self.cache_back += int(back.sum())
        self.rounds += 1

    def finish(self, post):
        nspan = self.span.numel()
        assert bool((self.next_hit == nspan).all())                              # hits 1, 2, ..., nspan - 1, each once
        assert bool((post.si[PN_ROWS_FINISHED] == 1).all()) and int(post.summary[0]) == 0
        assert torch.equal(post.sd[PN_ROWS_T], torch.full((self.B,), float(self.span[-1]), dtype=torch.float64))


class DenseInvariants:
    """Form B: over a solve the ranges [lo, hi) and the copies of a row cover the outputs 1 .. nout-1 once each, in order."""

    def __init__(self, B, times):
        self.B, self.times, self.nout = B, times, times.numel()
        self.cursor = torch.ones(B, dtype=torch.int64)
        self.landings = 0
        self.finals = 0

    def see(self, pre, post):
        nout, times = self.nout, self.times
        lo, hi, hit, nxt = post.range[0].long(), post.range[1].long(), post.log_hit.long(), post.next.long()
        acc = post.accept == 1
        tnew = post.sd[PN_ROWS_T]
        assert torch.equal(lo, self.cursor) and bool((hi >= lo).all()) and bool((hi[acc] <= nout - 1).all())
        assert bool(((hi == lo) & (hit == -1))[~acc].all())
        copied = hit >= 0
        assert torch.equal(hit[copied], hi[copied])                              # the copy follows the interpolated ones directly
        self.cursor = torch.where(copied, hi + 1, hi)
        assert torch.equal(nxt, self.cursor)
        # what was interpolated lies before the new time, what is left does not; a copy is the new time's own output
        some = hi > lo
        assert bool((times[(hi - 1).clamp(min=0)][some] < tnew[some]).all())
        assert bool((times[lo.clamp(max=nout - 1)][some] > pre.sd[PN_ROWS_T][some]).all())
        left = acc & ~copied
        assert bool((times[hi.clamp(max=nout - 1)][left] > tnew[left]).all())
        assert torch.equal(times[hit[copied]], tnew[copied])
        self.landings += int((copied & (hit < nout - 1)).sum())
        self.finals += int((hit == nout - 1).sum())

    def finish(self, post):
        assert bool((self.cursor == self.nout).all()) and self.finals == self.B


# ---------------------------------------------------------------------------------------------------------------- pow in play
POW_SPAN = torch.tensor([0.0, 0.013, 0.1, 0.11, 0.25, 0.4], dtype=torch.float64)
POW_TMAX = 0.4
POW_B = 300                                          # two workgroups, the second one ragged
POW_OPTIONS = {
    "safety": dict(ts_adapt_safety=0.8, ts_adapt_reject_safety=0.05),
    "dt_min": dict(ts_adapt_dt_min=0.004),           # above the steps of the rows that start small or were cut: norms above 1 pass
    "dt_max": dict(ts_adapt_dt_max=0.02),            # below what an accepted step of 0.012 or more grows to
}


def pow_h0(B):
    g = torch.Generator().manual_seed(B)
    return 0.001 + 0.011 * torch.rand(B, generator=g, dtype=torch.float64)       # never beyond the first output time


def pow_norms(B, k):
    """Lognormal around 0.05: one norm in fifteen rejects, so some rows are rejected twice in a row."""
    g = torch.Generator().manual_seed(1000 * B + k)
    return torch.exp(2.0 * torch.randn(B, generator=g, dtype=torch.float64)) * 0.05


def pow_branches(rounds, options):
    """How many row-rounds took the dt_min branch (accepted with a norm above 1), were clamped to dt_max, were rejected right
    after a rejection."""
    dt_min, dt_max = options.get("ts_adapt_dt_min", 1e-20), options.get("ts_adapt_dt_max", 1e50)
    forced = capped = again = 0
    for pre, enorm, post in rounds:
        was_open = pre.si[PN_ROWS_FINISHED] == 0
        acc = post.accept == 1
        forced += int((acc & (enorm > 1.0)).sum())
        rej = was_open & ~acc & (post.si[PN_ROWS_FAIL] == 0)
        # (an accepted row's clamped step may then be cut towards an output time: only the rows that kept it are counted)
        capped += int(((rej | acc) & (post.sd[PN_ROWS_H] == dt_max)).sum())
        again += int((was_open & ~acc & (pre.si[PN_ROWS_PREV_REJ] == 1)).sum())
        assert not bool((acc & (enorm > 1.0) & (pre.sd[PN_ROWS_H] >= (1.0 + 2.0 ** -26) * dt_min)).any())
    return forced, capped, again


# ---------------------------------------------------------------------------------------------------------------- one prepared round
SUMMARY_BATCHES = BATCHES + [70000]
SUMMARY_TMAX = 100.0                                 # out of reach: no row finishes by arriving
SUMMARY_STEPS = 7                                    # the step count every row comes with


def positions(B):
    """Row 0, the wave seam, the workgroup seam, the first row of the last workgroup, the last row: those that exist."""
    want = [0, WAVE - 1, WAVE, WG - 1, WG, (B - 1) // WG * WG, B - 1]
    return sorted({p for p in want if 0 <= p < B})


def summary_cases(B):
    """[(name, {row: failure code})]: each position alone (both codes over the list), all at once, and every pair with the
    codes (2, 1) and (1, 2) -- the earlier ROW must win, not the smaller code."""
    pos = positions(B)
    cases = [("none", {})]
    cases += [("row %d code %d" % (p, 1 + i % 2), {p: 1 + i % 2}) for i, p in enumerate(pos)]
    cases += [("row %d code %d" % (p, 2 - i % 2), {p: 2 - i % 2}) for i, p in enumerate(pos)]
    cases.append(("all", {p: 2 - i % 2 for i, p in enumerate(pos)}))
    for i, p in enumerate(pos):
        for q in pos[i + 1:]:
            cases.append(("rows %d, %d codes 2, 1" % (p, q), {p: 2, q: 1}))
            cases.append(("rows %d, %d codes 1, 2" % (p, q), {p: 1, q: 2}))
    return cases


def summary_base(B):
    """A state in mid-solve: a random third of the rows finished, the others with norms on either side of 1."""
    g = torch.Generator().manual_seed(B)
    st = new_state(B, 0.001 + 0.05 * torch.rand(B, generator=g, dtype=torch.float64), 0)
    st.sd[PN_ROWS_T] = 0.1 * torch.rand(B, generator=g, dtype=torch.float64)
    st.sd[PN_ROWS_TFIRST] = st.sd[PN_ROWS_T]
    st.si[PN_ROWS_STEPS] = SUMMARY_STEPS
    done = torch.rand(B, generator=g) < 1.0 / 3.0
    st.si[PN_ROWS_FINISHED] = done.to(torch.int32)
    st.sd[PN_ROWS_H][done] = 0.0
    enorm = torch.exp(2.0 * torch.randn(B, generator=g, dtype=torch.float64)) * 0.5
    return st, enorm


def summary_case(base, base_enorm, fails, h_open=0.01):
    """The base state with the rows of `fails` made to fail: code 1 by a NaN norm, code 2 by a norm above 1 on a row that has
    used up ts_max_reject.  Returns (state, norms)."""
    st, enorm = copy_state(base), base_enorm.clone()
    for r, code in fails.items():
        st.si[PN_ROWS_FINISHED][r] = 0
        st.sd[PN_ROWS_H][r] = h_open
        if code == 1:
            enorm[r] = float("nan")
        else:
            enorm[r] = 2.0
            st.si[PN_ROWS_REJ_STEP][r] = MAX_REJECT
            st.si[PN_ROWS_PREV_REJ][r] = 1
    return st, enorm


def summary_expect(pre, enorm, fails, max_steps=None):
    """(the summary, the rows' FINISHED codes) after one round, from the inputs alone: a failing row is finished with 3; with
    ts_max_steps = steps + 1 every accepted row (norm at most 1; dt_min is far below every step) is finished with 2; the final
    time is out of reach."""
    fin = pre.si[PN_ROWS_FINISHED].clone()
    for r in fails:
        fin[r] = 3
    if max_steps is not None:
        assert max_steps == SUMMARY_STEPS + 1
        fin[(pre.si[PN_ROWS_FINISHED] == 0) & (enorm <= 1.0)] = 2
    first = min(fails) if fails else -1
    return [int((fin == 0).sum()), first, fails[first] if fails else 0, 0], fin


def check_summary_round(pre, enorm, post, fails, max_steps=None):
    want, fin = summary_expect(pre, enorm, fails, max_steps)
    assert post.summary.tolist() == want, (post.summary.tolist(), want)
    assert torch.equal(post.si[PN_ROWS_FINISHED], fin)
    code = torch.zeros(pre.B, dtype=torch.int32)
    for r, c in fails.items():
        code[r] = c
    assert torch.equal(post.si[PN_ROWS_FAIL], code)
    rows = torch.tensor(sorted(fails), dtype=torch.int64)
    assert bool((post.sd[PN_ROWS_H][rows] == 0.0).all()) and bool((post.accept[rows] == 0).all())
    assert bool((post.log_d[0][rows] == 0.0).all()) and bool((post.log_hit[rows] == -1).all())
    was_open = pre.si[PN_ROWS_FINISHED] == 0
    ok = was_open & (code == 0)
    assert torch.equal(post.accept[ok] == 1, enorm[ok] <= 1.0)                   # a NaN elsewhere would show here
    assert bool((post.sd[PN_ROWS_H][fin != 0] == 0.0).all()) and bool((post.sd[PN_ROWS_H][fin == 0] > 0.0).all())
