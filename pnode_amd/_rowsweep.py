"""Per-sample adaptive step control (``-pn_adapt_scope sample``) as a mixin of ``ODEPetsc``.

The first dimension of the state is the batch: B rows of d entries.  Every row is integrated as the engine would integrate
it alone -- its own WRMS norm, time, step size, accept / reject and MATCHSTEP approach to every output time -- but all rows
advance together in ROUNDS: one step attempt of every unfinished row, with func called once per stage for the whole batch
(``t`` is a float64 tensor of shape (B, 1, ..., 1)).  The per-row controller runs on the device (pn_rows_control: the text of
pn_ts_judge); the host reads one small summary per round.  The round log (per round and row: h_eff = the step size where the
attempt was accepted, else 0; the times; the output index the row landed on) is all the reverse sweep needs: a round with
h_eff = 0 is the identity on that row in both sweeps, so the rounds are reversed in order with no per-row control flow.

With ``-pn_output_times interpolate`` (a backend with the row-dense entry points, ``rows_dense``) the controller sees
``[t[0], t[-1]]`` only: every row takes the steps its own tolerance asks for, and after each round pn_rows_dense_eval fills the
output times an accepted attempt has passed from the tableau's continuous extension (the output times and a per-row "next
output" counter live on the device; the round's log grows by the range [lo, hi) of outputs each row interpolated).

dL/dt (``t.requires_grad``, a backend with ``rows_tgrad``): every row's dL/dt is DESIGN.md section 5.6's rule on its own logged
steps.  Per reversed round the rows' <w_j, K_j> and <w_j, df/dt> are gathered on the device and pn_rows_tgrad_scatter sends them
into the row's own column of an fp64 [T][B] matrix (``sample_time_grads``); one ordered sum over the rows at the end is t.grad.

``-pn_rows_compact 1`` (a backend with ``rows_compact``): func is evaluated, and differentiated, on the rows of a round that have
work to do -- forward the rows still unfinished at the round's start, backward the rows whose attempt was accepted (h_eff > 0).
pn_rows_list writes the ordered list, pn_rows_gather packs the stage value, the times and the cotangent of those rows into a dense
sub-batch of m <= B rows, pn_rows_scatter writes func's result (J^T w, <w, df/dt>) back into a full-size buffer whose other rows
are +0.  Every pn_rows_* kernel of the step itself stays at full size."""
import collections
import ctypes
import types
import warnings

import torch

from . import _lib
from ._lib import PN_ROWS_CACHED, PN_ROWS_H, PN_ROWS_REJ, PN_ROWS_SPANCTR, PN_ROWS_STEPS, PN_ROWS_T, PN_ROWS_TFIRST, PnError, check

_LOG_BLOCK = 64          # rounds per allocation of the round log

# One round of the log, an entry per row in every field: h_eff, the time and the first-stage time at the round's start (`log_d`: the
# packed [3][B] tensor of the three, as the entry points take it), the output the row landed on or -1, [2][B] the outputs [lo, hi) it interpolated,
# and under -pn_rows_compact 1 [2][B] the list of the rows with h_eff > 0 (idx, pos: what the reversed round gathers and scatters by)
_Round = collections.namedtuple("_Round", "heff t tfirst hit range log_d lists")


class _RoundLog(object):
    """The rounds of a per-sample solve, allocated _LOG_BLOCK rounds at a time (the range block only with interpolated outputs, the
    list block only where a reverse sweep under -pn_rows_compact 1 will read it).  `counts`: with lists, ONE device int32 array of
    the lists' lengths, a round an entry (it doubles when it is full); the reverse sweep reads it once."""

    def __init__(self, ops, B, ranges, lists=False):
        self._new = lambda: (ops.f64(_LOG_BLOCK, 3, B), ops.i32(_LOG_BLOCK, B), ops.i32(_LOG_BLOCK, 2, B) if ranges else None,
                             ops.i32(_LOG_BLOCK, 2, B) if lists else None)
        self._blocks, self._n = [], 0
        self._i32 = ops.i32
        self.counts = ops.i32(_LOG_BLOCK) if lists else None

    def append(self):
        if self._n % _LOG_BLOCK == 0:
            self._blocks.append(self._new())
        if self.counts is not None and self._n == self.counts.numel():
            grown = self._i32(2 * self._n)
            grown[: self._n] = self.counts
            self.counts = grown
        self._n += 1
        return self[self._n - 1]

    def __getitem__(self, k):
        log_d, hit, rng, lists = self._blocks[k // _LOG_BLOCK]
        i = k % _LOG_BLOCK
        d = log_d[i]
        return _Round(d[0], d[1], d[2], hit[i], None if rng is None else rng[i], d, None if lists is None else lists[i])


# the rows a func call works on under -pn_rows_compact 1: m of them, idx their numbers in ascending order, pos the inverse
_Sub = collections.namedtuple("_Sub", "m idx pos")


class RowSweep(object):
    _sample = False
    _rows_probe = False
    _rdense = None           # the last per-sample solve interpolated its outputs: its device-side plan
    rounds = 0
    sample_steps = None
    sample_rejections = None
    sample_time_grads = None      # after a backward with t.requires_grad: fp64 [T][B], what row r sends to dL/dt_i (its sum over r is t.grad)
    _compact = False              # -pn_rows_compact 1
    # the rows passed to func, summed over the calls nfe_forward / nfe_backward count (from the solver's creation, as they are);
    # without -pn_rows_compact 1 every call passes the B rows of the batch
    rows_evaluated = 0
    rows_evaluated_backward = 0
    _rows_full = (0, 0)           # what the two would be with every call at full size

    # ------------------------------------------------------------------ surface
    def _rows_refusals(self):
        """What -pn_adapt_scope sample is not built for is refused by name (setupTS), never served by another path."""
        opt = "-pn_adapt_scope sample"
        if self._stepper_kind:
            raise PnError("%s is built for the explicit RK steppers; the %s stepper takes -pn_adapt_scope batch" % (opt, self._stepper_kind))
        if not self._adaptive:
            raise PnError("%s needs an adaptive scheme: a tableau with an embedded pair (2a, 2b, 3bs, 5f, 5dp) and "
                          "-ts_adapt_type basic" % opt)
        if len(self.tensor_size) < 2:
            raise PnError("%s: the first dimension of the state is the batch; a 1-D state has no rows to control" % opt)
        if self._dense and not getattr(self._ops, "rows_dense", False):
            # (a tableau without a continuous extension has been refused by ts_tableau_dense before)
            raise PnError("%s cannot be combined with -pn_output_times interpolate on this backend" % opt)
        if self._max_cps > 0:
            raise PnError("%s cannot be combined with -ts_trajectory_max_cps_ram / -ts_trajectory_max_cps_disk" % opt)
        if self._traj_disk:
            raise PnError("%s cannot be combined with -ts_trajectory_type basic" % opt)
        if isinstance(self.step_size, list):
            raise PnError("%s: a list step_size prescribes the steps of the whole batch; give one initial step size" % opt)
        if self._compact and not getattr(self._ops, "rows_compact", False):
            raise PnError("-pn_rows_compact 1 is not built on this backend (no pn_rows_list / pn_rows_gather / pn_rows_scatter); "
                          "%s runs with -pn_rows_compact 0" % opt)

    def _rows_compact_from_options(self, db):
        """-pn_rows_compact 0|1 (not a PETSc option): 1 evaluates and differentiates func on the rows of a
        round that have work to do.  Unknown pn_* keys are skipped by _set_from_options, so the value is checked here."""
        val = str(db.get("pn_rows_compact", "0"))
        if val not in ("0", "1"):
            raise PnError("-pn_rows_compact must be 0 or 1 (got '%s')" % val)
        self._compact = val == "1"
        if self._compact and not self._sample:
            raise PnError("-pn_rows_compact 1 needs -pn_adapt_scope sample: only a per-sample solve has rows that finish, or are "
                          "rejected, on their own")

    @property
    def rows_compact(self):
        """Status of -pn_rows_compact: "off", or the rows func was called with against what full-size calls would have passed."""
        if not self._compact:
            return "off"
        return ("on (rows evaluated %d of %d forward, %d of %d backward)"
                % (self.rows_evaluated, self._rows_full[0], self.rows_evaluated_backward, self._rows_full[1]))

    def _graph_entry(self, y0, t, need):
        if self._sample:
            self._graph_status = "eager (-pn_adapt_scope sample: the rounds of a per-sample solve are launched eagerly)"
            return None
        return super(RowSweep, self)._graph_entry(y0, t, need)

    def _tgrad_supported(self):
        if self._sample:
            if getattr(self._ops, "rows_tgrad", False):
                return super(RowSweep, self)._tgrad_supported()          # (-pn_reference_defaults keeps the reference's None)
            if not self._tg_warned:
                self._tg_warned = True
                warnings.warn("pnode_amd: the gradient with respect to the output times t is not built under -pn_adapt_scope "
                              "sample; None is returned for it", RuntimeWarning, stacklevel=4)
            return False
        return super(RowSweep, self)._tgrad_supported()

    def _setup_linear_grads(self):
        if self._sample:
            # the parameter cotangents of a round come from autograd on the row-prescaled stage cotangents: the engine-side
            # Linear path scales a whole stage by one scalar, which a per-row step size is not
            if self._lin is not None:
                self._lin.remove()
            self._lin, self._lin_sig = None, None
            self._fwd, self._fwd_sig = None, None
            return
        return super(RowSweep, self)._setup_linear_grads()

    @property
    def linear_param_grads(self):
        if self._sample:
            return "autograd (-pn_adapt_scope sample: per-row step sizes are folded into the stage cotangents, the engine-side Linear path is off)"
        return super(RowSweep, self).linear_param_grads

    def sample_step_log(self, row):
        """[(t_n, h_n)] of the accepted steps of `row` in the last -pn_adapt_scope sample solve."""
        out = []
        for k in range(self.rounds):
            rnd = self._round_log[k]
            h = float(rnd.heff[row])
            if h > 0.0:
                out.append((float(rnd.t[row]), h))
        return out

    # ------------------------------------------------------------------ helpers
    def _rows_func(self, tvec, y_flat, tape=None, sub=None):
        """evalRHSFunction for the whole batch with per-row times; with `tape` (a list) recorded by autograd.  The time argument
        of func: float64, one entry per row, broadcastable against the state.  With `sub` (-pn_rows_compact 1, fewer than B rows
        have work to do) func sees those rows only, state (m, ...) and times (m, 1, ..., 1), and the result is a full-size buffer
        whose other rows are +0; the tape is the sub-batch's."""
        B, d = self._rB, self.n // self._rB
        if sub is not None:
            ops, m = self._ops, sub.m
            y_full, y_flat = y_flat, ops.empty(m * d)
            ops.rows_gather(m, d, y_flat, y_full, sub.idx)
            t_full, tvec = tvec, tvec.new_empty(m)
            ops.rows_gather(m, 1, tvec, t_full, sub.idx)
            y = y_flat.view((m,) + tuple(self.tensor_size[1:]))
        else:
            m = B
            y = self._shaped(y_flat)
        targ = tvec.view((m,) + (1,) * (len(self.tensor_size) - 1))
        back = tape is not None
        self.rows_evaluated, self.rows_evaluated_backward = self.rows_evaluated + (0 if back else m), self.rows_evaluated_backward + (m if back else 0)
        self._rows_full = (self._rows_full[0] + (0 if back else B), self._rows_full[1] + (B if back else 0))
        try:
            if tape is not None:
                with torch.enable_grad():
                    y = y.detach().requires_grad_(True)
                    if self._tgrad:
                        # dL/dt: the rows' times are one more leaf of this evaluation (its gradient: <w, df/dt> per row)
                        targ = targ.detach().requires_grad_(True)
                    k, wrt = self._func_with_grad(targ, y)
                tape.append((y, k, wrt, targ) if self._tgrad else (y, k, wrt))
            else:
                k = self.funcEX(targ, y)
        except Exception as exc:
            if self._rows_probe:
                # the first evaluation of a solve failed: a func that runs with a host number for t but not with one time
                # per row is told so (decided by calling it, not by the exception's wording)
                self._rows_probe = False
                try:
                    with torch.no_grad():
                        self.funcEX(float(targ.reshape(-1)[0]), self._shaped(y_flat))
                except Exception:
                    raise exc from None
                raise PnError("-pn_adapt_scope sample calls func with t as a float64 tensor of shape (B, 1, ..., 1), one time per "
                              "row; this func runs with a host number for t only (float(t) / t.item() inside it?): %s: %s"
                              % (type(exc).__name__, exc)) from exc
            raise
        self._rows_probe = False
        if sub is None:
            return self._func_result(k, y_flat)
        full = self._ops.empty(self.n)
        self._ops.rows_scatter(B, d, full, self._func_result(k, y_flat, m * d), sub.pos)
        return full

    def _rows_stages(self, stages, Y, held, h, t, tfirst, tapes=None, sub=None):
        """K_i = f(t_r + c_i h_r, Y_i) for `stages` in order, the whole batch per call.  Y[0] is the round's state, evaluated at the rows'
        first-stage times; Y_i = u + h_r sum_j a_ij K_j is formed into Y[i] unless it is `held` there already.  With `tapes` (a dict)
        the evaluations are the reverse sweep's, recorded by autograd: tapes[i] = (input, output, parameters).  `sub`: the rows func
        is called with (_rows_func); the stage values are formed at full size all the same."""
        A, K = self._A, {}
        for i in stages:
            if i and i not in held:
                idx = [j for j in range(i) if A[i][j] != 0.0]
                self._ops.rows_stage(self._rB, self.n // self._rB, Y[i], Y[0], [K[j] for j in idx], [A[i][j] for j in idx], h)
            rec = None if tapes is None else []
            K[i] = self._rows_func(t + self._c[i] * h if i else tfirst.clone(), Y[i], rec, sub)
            if tapes is None:
                self.nfe_forward += 1
            else:
                tapes[i] = rec[0]
                self.nfe_backward += 1
        return K

    # ------------------------------------------------------------------ forward rounds
    def _rows_odeint(self, u0, t, save):
        st = self._rows_begin(u0, t, save)
        if st.tmax > st.t0:
            while self._rows_round(st):
                pass
        else:
            # nothing to integrate (one output time at or before 0; pn_ts_begin has refused a span that does not increase)
            for i in range(st.T):
                self._ops.copy(st.sol[i], st.u0)
            st.si[PN_ROWS_SPANCTR].fill_(st.T)
        # per row, the number of output times it has reached: the rows' own counter, or the controller's span counter
        served = st.si[PN_ROWS_SPANCTR] if st.dense is None else st.dense.next
        host = st.si.cpu()
        self.sample_steps = host[PN_ROWS_STEPS].clone()
        self.sample_rejections = host[PN_ROWS_REJ].clone()
        self._nsteps = int(self.sample_steps.max()) if st.B else 0
        if st.T > 1:
            short = (served.cpu() != st.T).nonzero()
            if short.numel():
                raise Exception("TSSolve fails to step on all the specified points (-pn_adapt_scope sample: row %d)" % int(short[0]))
        if self._view and self.rounds:
            print("TS Object (pnode_amd): type rk, -pn_adapt_scope sample: %d rounds for %d rows, accepted steps per row %d..%d, "
                  "rejected %d..%d; output times: %s; launches: %s%s"
                  % (self.rounds, st.B, int(self.sample_steps.min()), int(self.sample_steps.max()),
                     int(self.sample_rejections.min()), int(self.sample_rejections.max()),
                     "interpolate (per row, continuous extension of order %d)" % self._dense_order if st.dense is not None else "match",
                     self._graph_status, "; -pn_rows_compact: " + self.rows_compact if self._compact else ""))
        return st.solution

    def _rows_begin(self, u0, t, save):
        """The state of a forward sweep: the span as the controller sees it, the controllers' rows seeded from the host engine's
        first attempt, the buffers the rounds turn over and, with interpolated outputs, the rows' device-side plan."""
        lib, ops, ts = self._lib, self._ops, self._ts
        B = self._rB = int(self.tensor_size[0])
        n = self.n
        self.sol_times = t.detach().cpu().to(dtype=torch.float64)
        times = self.sol_times.tolist()
        T = len(times)
        st = types.SimpleNamespace(B=B, d=n // B, T=T, save=save, dense=None)
        st.solution = ops.empty((T,) + tuple(self.tensor_size))
        st.sol = st.solution.view(T, -1)
        st.u0 = u0.detach().contiguous().reshape(-1)
        # -pn_output_times interpolate: the controller sees the end points only; t[1:-1] are filled by rows_dense_eval
        self._rdense = None
        if self._dense and T > 2:
            if any(not (b > a) for a, b in zip(times, times[1:])):
                raise PnError("-pn_output_times interpolate: the output times must be strictly increasing")
            cols = self._dense_cols
            pv = [v for j in cols for v in list(self._dense_P[j]) + [0.0] * (_lib.PN_DENSE_MAX_POW - len(self._dense_P[j]))]
            st.dense = self._rdense = types.SimpleNamespace(times=self.sol_times.to(self.device), cols=cols,
                                                            P=(ctypes.c_double * len(pv))(*pv), next=ops.i32(B))
            st.dense.next.fill_(1)               # times[0] is the initial condition itself
            times = [times[0], times[-1]]
        # the first step of every row: the host engine's own MATCHSTEP clamp at the start of a solve (pn_ts_begin)
        nt = len(times)
        check(lib.pn_ts_begin(ts, 0.0, float(self.step_size), nt, (ctypes.c_double * nt)(*times)))
        st.t0, st.tmax = (0.0 if nt == 1 else times[0]), times[-1]
        # -pn_rows_compact 1: the forward rounds' list of open rows (rewritten every round) and, where a reverse sweep follows, every
        # round's list of stepped rows in the log
        st.compact = self._compact
        st.nopen = B
        st.lists = ops.i32(2, B) if st.compact else None
        st.nlist = ops.i32(1) if st.compact else None
        self._round_log = _RoundLog(ops, B, st.dense is not None, st.compact and save)
        # the stage values of every round are kept for the reverse sweep, or live in scratch that every round rewrites
        st.store = save and not self._solution_only and not self._solution_only_auto
        self._rtraj, self._rY = ([] if save else None), ([] if st.store else None)
        self._rows_probe = True                    # the first evaluation of this solve is still to come
        self.rounds = 0
        st.sd, st.si = ops.f64(_lib.PN_ROWS_ND, B), ops.i32(_lib.PN_ROWS_NI, B)
        st.cur = ops.empty(n)
        ops.copy(st.cur, st.u0)
        if T > 1:
            ops.copy(st.sol[0], st.u0)
        if not st.tmax > st.t0:
            return st
        tt, hh = ctypes.c_double(), ctypes.c_double()
        check(lib.pn_ts_attempt(ts, ctypes.byref(tt), ctypes.byref(hh)))
        st.sd[PN_ROWS_T].fill_(tt.value)
        st.sd[PN_ROWS_H].fill_(hh.value)
        st.sd[PN_ROWS_TFIRST].fill_(tt.value)
        st.sd[PN_ROWS_CACHED].fill_(lib.pn_ts_span_cached_dt(ts))
        if nt > 1:
            st.si[PN_ROWS_SPANCTR].fill_(1)      # times[0] is the initial condition itself
        st.nspan, st.span = (nt, torch.tensor(times, dtype=torch.float64).to(self.device)) if nt > 1 else (0, None)
        st.enorm, st.accept, st.summary = ops.f64(B), ops.i32(B), ops.i32(4)
        st.ie = [j for j in range(self._s) if self._e[j] != 0.0 or (not self._fsal and self._b[j] != 0.0)]    # the stages of the error estimate
        st.scratch = None if st.store else [ops.empty(n) for _ in range(self._s)]
        st.unew = [ops.empty(n), ops.empty(n)]
        if not save:
            st.pingpong = [ops.empty(n), st.cur]   # the states of successive rounds, in turn
        if self._monitor:
            print("round %d: t [%g, %g] dt [%g, %g] rows unfinished %d" % (0, tt.value, tt.value, hh.value, hh.value, B))
        return st

    def _rows_round(self, st):
        """One step attempt of every unfinished row: the stages, the rows' error norms, the controllers' judgement, the outputs
        the accepted attempts serve and the next round's state.  Returns the number of rows still unfinished."""
        ops, B, d, n = self._ops, st.B, st.d, self.n
        b, e, fsal = self._b, self._e, self._fsal
        sd, cur, k = st.sd, st.cur, self.rounds
        log = self._round_log.append()
        h, tr = sd[PN_ROWS_H], sd[PN_ROWS_T]
        unew = st.unew[k % 2]
        Y = [cur] + ([ops.empty(n) for _ in range(1, self._s_eff)] if st.store else st.scratch[1:self._s_eff])
        # (first same as last: the last stage value is the new state itself)
        sub = None
        if st.compact and st.nopen < B:
            # the rows unfinished at this round's start: their number is what the last round's summary read back
            ops.rows_list(B, 0, st.si[_lib.PN_ROWS_FINISHED], st.lists[0], st.lists[1], st.nlist)
            sub = _Sub(st.nopen, st.lists[0], st.lists[1])
        K = self._rows_stages(range(self._s), Y + [unew] if fsal else Y, (), h, tr, sd[PN_ROWS_TFIRST], None, sub)
        self._err_rows_combine(B, d, None if fsal else unew, unew if fsal else cur, [K[j] for j in st.ie],
                               [b[j] for j in st.ie], [e[j] for j in st.ie], h, st.enorm)
        ops.rows_control(self._ts, B, st.nspan, st.span, st.tmax, st.enorm, sd, st.si, log.log_d, log.hit, st.accept, st.summary)
        if log.lists is not None:
            # what the reversed round will work on: the rows this attempt moved (h_eff > 0); the count stays on the device
            ops.rows_list(B, 1, log.heff, log.lists[0], log.lists[1], self._round_log.counts[k:k + 1])
        if st.save:
            nxt = ops.empty(n)
            self._rtraj.append(cur)
            if st.store:
                self._rY.append(Y)
        else:
            nxt = st.pingpong[k % 2]
        if st.dense is not None:
            # the outputs this round's accepted attempts have passed, and the copies of the new state (an exact landing, the
            # final time): log.hit becomes the output copied, as the reverse sweep's masked forcing reads it
            dn = st.dense
            ops.rows_dense_eval(B, d, st.sol, dn.times, cur, [K[j] for j in dn.cols], dn.P, unew, log.log_d, sd[PN_ROWS_T], log.hit,
                                dn.next, log.range)
            ops.rows_commit(B, d, nxt, cur, unew, st.accept, None, None, 0, 0)
        else:
            ops.rows_commit(B, d, nxt, cur, unew, st.accept, log.hit, st.sol, n, st.T)
        st.cur = nxt
        self.rounds = k + 1
        nopen, frow, fcode = ops.rows_summary(st.summary)          # the one read-back of the round
        st.nopen = nopen
        if frow >= 0:
            self._lib.pn_rows_failure(fcode, frow)
            raise PnError(self._lib.pn_last_error().decode())
        if self._monitor:
            print("round %d: t [%g, %g] dt [%g, %g] rows unfinished %d"
                  % (k + 1, float(sd[PN_ROWS_T].min()), float(sd[PN_ROWS_T].max()), float(sd[PN_ROWS_H].min()),
                     float(sd[PN_ROWS_H].max()), nopen))
        return nopen

    # ------------------------------------------------------------------ reverse rounds
    def _rows_reverse(self, g, T):
        """The exact discrete adjoint of the logged per-row step sequences (step sizes held constant): the rounds in reverse,
        row r of round k with the logged h_eff[k][r]."""
        if self._rtraj is None:
            raise RuntimeError("adjoint requested but no trajectory was saved "
                               "(setupTS(enable_adjoint=True) and a differentiable input are required)")
        ops, log = self._ops, self._round_log
        B, n, d, dn = self._rB, self.n, self.n // self._rB, self._rdense
        # the stages of a reversed round.  With interpolated outputs whose extension uses the last stage of a first-same-as-last
        # tableau, that stage is an ordinary one here (nothing is routed between rounds: stage 0 is re-evaluated every round):
        # Y_{s-1} = u + h sum_j a_{s-1,j} K_j, cotangent D_{s-1} alone -- one more evaluation and VJP per reversed round
        stages = list(range(self._s_eff))
        if dn is not None and self._fsal and (self._s - 1) in dn.cols:
            stages.append(self._s - 1)
        lam = self.adj_u_tensor = self.adj_u_flat = ops.empty(n)
        lam.zero_()
        self._begin_param_adjoint()
        g = g.contiguous()
        ld = g.stride(0)
        R = self.rounds
        tg = self._rows_tg_begin(T) if self._tgrad else None
        # -pn_rows_compact 1: how many rows every round moved -- the one read-back of this sweep
        moved = log.counts[:R].tolist() if log.counts is not None and R else None
        if R == 0:
            ops.rows_adj_accum(B, d, lam, lam, [], g, ld, ops.i32(B), T)
            self._rows_tg_end(tg)
            return
        hit0 = ops.i32(B) if T > 1 else None           # every row's state at t[0] is u0
        ops.rows_adj_accum(B, d, lam, lam, [], g, ld, log[R - 1].hit, T)
        rv = types.SimpleNamespace(stages=stages, lam=lam, w=ops.empty(n), y=[None] + [ops.empty(n) for _ in range(1, stages[-1] + 1)],
                                   D=dict((j, ops.empty(n)) for j in (dn.cols if dn is not None else ())), G=ops.empty(n) if dn is not None else None)
        for k in range(R - 1, -1, -1):
            rnd = log[k]
            # the round's stage evaluations again, recorded by autograd: on the stage values the forward sweep kept, else on
            # ones recomputed from the round's state with the logged h_eff
            kept = self._rY[k] if self._rY is not None else [self._rtraj[k]]
            sub = _Sub(moved[k], rnd.lists[0], rnd.lists[1]) if moved is not None and moved[k] < B else None
            if sub is not None and sub.m == 0:
                # every open row was rejected in this round: the identity on every row.  Nothing is evaluated or differentiated and
                # the stage cotangents are zero; what is left is the forcing of the output the previous round landed on, and the
                # dL/dt bookkeeping (every row has h_eff = 0: nothing is sent)
                if tg is not None:
                    tg.tbar = {}
                    self._rows_tg_round(tg, rnd, g, None)
                hit_prev = log[k - 1].hit if k > 0 else hit0
                ops.rows_adj_accum(B, d, lam, lam, [], g if hit_prev is not None else None, ld, hit_prev, T)
                self._rtraj[k] = None
                if self._rY is not None:
                    self._rY[k] = None
                continue
            tapes = {}
            K = self._rows_stages(stages, kept + rv.y[len(kept):], range(len(kept)), rnd.heff, rnd.t, rnd.tfirst, tapes, sub)
            if tg is not None:
                tg.K, tg.first, tg.tbar = K, True, {}
            if dn is not None:
                # D_j[r] = sum_o h_r beta_j(theta_o) g[o, r] over the outputs row r interpolated in this round, G[r] = sum_o g[o, r]
                ops.rows_dense_adjoint(B, d, [rv.D[j] for j in dn.cols], rv.G, g, dn.times, dn.P, rnd.range, rnd.log_d)
            dlam = [None] * self._s
            for i in reversed(stages):
                w = self._rows_cotangent(rv, i, dlam, rnd.heff)
                if w is not None:
                    dlam[i] = self._rows_vjp(tapes, i, w, tg, sub)
            self._flush_param_accum()
            if tg is not None:
                self._rows_tg_round(tg, rnd, g, K)
            # lambda += sum_i dlam_i (+ G) (+ g at the output the previous round landed on), at most PN_MAX_STAGES terms a launch
            terms = [dlam[i] for i in stages if dlam[i] is not None]
            if dn is not None:
                terms.append(rv.G)
            if len(terms) > _lib.PN_MAX_STAGES:          # (5dp with interpolated outputs: seven stages and G)
                ops.rows_adj_accum(B, d, lam, lam, terms[_lib.PN_MAX_STAGES:], None, ld, None, T)
                terms = terms[: _lib.PN_MAX_STAGES]
            hit_prev = log[k - 1].hit if k > 0 else hit0
            ops.rows_adj_accum(B, d, lam, lam, terms, g if hit_prev is not None else None, ld, hit_prev, T)
            self._rtraj[k] = None
            if self._rY is not None:
                self._rY[k] = None
        self._flush_param_accum()
        self._rows_tg_end(tg)

    def _rows_cotangent(self, rv, i, dlam, heff):
        """Stage i's cotangent w_i[r] = h_r (b_i lambda[r] + sum_{j>i} a_ji dlam_j[r]) (+ D_i[r], what the row's interpolated
        outputs send the stage); None when it is structurally zero."""
        A, b = self._A, self._b
        js = [j for j in rv.stages if j > i and A[j][i] != 0.0 and dlam[j] is not None]
        Di = rv.D.get(i)
        if b[i] == 0.0 and not js:
            return Di                                # (the stage's cotangent is what its outputs send it, if anything)
        kw = {} if Di is None else {"dense_w": Di}
        self._ops.rows_adj_theta(self._rB, self.n // self._rB, rv.w, rv.lam if b[i] != 0.0 else None, b[i], [dlam[j] for j in js],
                                 [A[j][i] for j in js], heff, **kw)
        return rv.w

    def _rows_vjp(self, tapes, i, w, tg=None, sub=None):
        """The backward half of stage i with cotangent `w`: returns J^T w; the parameter cotangents are queued for mu.  With `tg`
        (this backward computes dL/dt) the rows' <w, K_i> are taken first -- the cotangent buffer is rewritten for the next
        stage -- and the rows' times are one more input of autograd.grad: their gradient is <w, df/dt> per row.  With `sub` the tape
        is the sub-batch's: the cotangent's rows are gathered for it, and J^T w and <w, df/dt> are scattered into full-size buffers of
        their own (the other rows +0)."""
        y, out, wrt = tapes[i][:3]
        tt = () if tg is None else (tapes[i][3],)
        tapes[i] = None
        if tg is not None:
            self._ops.rows_tgrad_dots(self._rB, self.n // self._rB, tg.rowacc, [w], [tg.K[i]], [1.0], accumulate=not tg.first)
            tg.first = False
        if sub is not None:
            ops, B, d = self._ops, self._rB, self.n // self._rB
            wc = ops.empty(sub.m * d)
            ops.rows_gather(sub.m, d, wc, w, sub.idx)
            grads = torch.autograd.grad(out, (y,) + tuple(wrt) + tt, wc.view(out.shape), allow_unused=True)
            if tt:
                gt, grads = grads[-1], grads[:-1]
                if gt is not None:
                    tg.tbar[i] = gt.new_empty(B, dtype=torch.float64)
                    ops.rows_scatter(B, 1, tg.tbar[i], gt.to(torch.float64).contiguous().reshape(-1), sub.pos)
            # (the gathered cotangent is this stage's alone and is not rewritten: nothing that shares its storage needs a copy)
            gc, gp = self._vjp_results(grads[0], grads[1:], wc, deferred=False)
            gy = None
            if gc is not None:
                gy = ops.empty(self.n)
                ops.rows_scatter(B, d, gy, gc, sub.pos)
            self._take_param_grads(1.0, gp)
            return gy
        grads = torch.autograd.grad(out, (y,) + tuple(wrt) + tt, self._shaped(w).view(out.shape), allow_unused=True)
        if tt:
            gt, grads = grads[-1], grads[:-1]
            if gt is not None:                       # (None: func's output does not reach t -- nothing is launched for it)
                tg.tbar[i] = gt.to(torch.float64).contiguous().reshape(-1)
        gy, gp = self._vjp_results(grads[0], grads[1:], w)
        if gy is not None and gy.untyped_storage().data_ptr() == w.untyped_storage().data_ptr():
            gy = gy.clone()
        self._take_param_grads(1.0, gp)           # (the row's h is inside the cotangent; one launch per round)
        return gy

    # ------------------------------------------------------------------ dL/dt
    def _rows_tg_begin(self, T):
        """The accumulators of a reverse sweep that returns dL/dt: dtrow [T][B] (row r's share of every dL/dt_i), the rows' sums of a
        round, and per row the output interval it is in and the first-stage scalar held for its previous accepted step."""
        ops, B, dn = self._ops, self._rB, self._rdense
        tg = types.SimpleNamespace(dtrow=ops.f64(T, B), rowacc=ops.f64(B), held=ops.f64(B), iv=ops.i32(B), K=None, first=True, tbar={},
                                   erow=ops.f64(T, B) if dn is not None else None)
        tg.iv.fill_(T - 1)
        return tg

    def _rows_tg_round(self, tg, rnd, g, K):
        """A reversed round's share of dL/dt, once its stage VJPs have run: the interpolated outputs' e_o, then the scatter into the
        rows' columns of dtrow (pn_rows_dense_tgrad, pn_rows_tgrad_scatter)."""
        ops, B, dn = self._ops, self._rB, self._rdense
        if dn is not None and K is not None:         # (K None: no row moved in this round, no output of it was interpolated)
            ops.rows_dense_tgrad(B, self.n // B, tg.erow, g, [K[j] for j in dn.cols], dn.times, dn.P, rnd.range, rnd.log_d)
        own = [j for j in sorted(tg.tbar) if not (self._fsal and j == 0)]
        ops.rows_tgrad_scatter(B, tg.dtrow, tg.rowacc, [tg.tbar[j] for j in own], [self._c[j] for j in own],
                               tg.tbar.get(0) if self._fsal else None, self._c[self._s - 1], self._fsal, rnd.log_d, rnd.hit,
                               rnd.range if dn is not None else None, tg.erow, dn.times if dn is not None else None, tg.held, tg.iv)

    def _rows_tg_end(self, tg):
        """After the last reversed round: what the rows still hold goes to t[0], then the one ordered sum over the rows."""
        if tg is None:
            return
        ops, B = self._ops, self._rB
        ops.rows_tgrad_scatter(B, tg.dtrow, None, [], [], None, 0.0, self._fsal, None, None, None, None, None, tg.held, tg.iv, flush=True)
        acc = ops.f64(tg.dtrow.shape[0])
        ops.rows_tgrad_reduce(B, tg.dtrow, acc)
        self.sample_time_grads = tg.dtrow
        self._tg = dict(acc=acc, rows=True)         # (over batch shards `acc` is summed with mu: ODEPetsc._allreduce_adj_p)

    def _tg_finish(self, t):
        if self._tg is not None and self._tg.get("rows"):
            tg, self._tg = self._tg, None
            return tg["acc"].to(dtype=t.dtype, device=t.device).view_as(t)
        return super(RowSweep, self)._tg_finish(t)
