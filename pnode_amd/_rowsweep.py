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
output" counter live on the device; the round's log grows by the range [lo, hi) of outputs each row interpolated)."""
import ctypes
import warnings

import torch

from . import _lib
from ._lib import PnError, check

_LOG_BLOCK = 64          # rounds per allocation of the round log


class RowSweep(object):
    _sample = False
    _rows_probe = False
    _rdense = False          # the last per-sample solve interpolated its outputs
    rounds = 0
    sample_steps = None
    sample_rejections = None

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

    def _graph_entry(self, y0, t, need):
        if self._sample:
            self._graph_status = "eager (-pn_adapt_scope sample: the rounds of a per-sample solve are launched eagerly)"
            return None
        return super(RowSweep, self)._graph_entry(y0, t, need)

    def _tgrad_supported(self):
        if self._sample:
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
            ld, _ = self._rows_log_at(k)
            h = float(ld[0, row])
            if h > 0.0:
                out.append((float(ld[1, row]), h))
        return out

    # ------------------------------------------------------------------ helpers
    def _rows_log_at(self, k):
        blk = self._rlog[k // _LOG_BLOCK]
        return blk[0][k % _LOG_BLOCK], blk[1][k % _LOG_BLOCK]

    def _rows_range_at(self, k):
        """int32 [2][B]: the outputs [lo, hi) every row interpolated in round k (-pn_output_times interpolate)."""
        return self._rlog[k // _LOG_BLOCK][2][k % _LOG_BLOCK]

    def _rows_t(self, tvec):
        """The time argument of func: float64, one entry per row, broadcastable against the state."""
        return tvec.view((self._rB,) + (1,) * (len(self.tensor_size) - 1))

    def _rows_func(self, targ, y_flat, tape=None):
        """evalRHSFunction for the whole batch with per-row times; with `tape` (a list) recorded by autograd."""
        y = self._shaped(y_flat)
        try:
            if tape is not None:
                with torch.enable_grad():
                    y = y.detach().requires_grad_(True)
                    k, wrt = self._func_with_grad(targ, y)
                tape.append((y, k, wrt))
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
        if k.dtype != self.tensor_dtype or k.device != self.device or k.numel() != self.n:
            raise ValueError("func must return a tensor with the state's shape, dtype and device")
        kd = k.detach()
        if not kd.is_contiguous():
            kd = kd.contiguous()
        if kd.untyped_storage().data_ptr() == y_flat.untyped_storage().data_ptr():
            kd = kd.clone()
        return kd.reshape(-1)

    # ------------------------------------------------------------------ forward rounds
    def _rows_odeint(self, u0, t, save):
        lib, ops, ts = self._lib, self._ops, self._ts
        B = self._rB = int(self.tensor_size[0])
        n = self.n
        d = n // B
        s, A, b, c, e = self._s, self._A, self._b, self._c, self._e
        self.sol_times = t.detach().cpu().to(dtype=torch.float64)
        T = int(t.shape[0])
        times = self.sol_times.tolist()
        dt0 = float(self.step_size)
        solution = ops.empty((T,) + tuple(self.tensor_size))
        sol_flat = solution.view(T, -1)
        u0f = u0.detach().contiguous().reshape(-1)
        # -pn_output_times interpolate: the controller sees the end points only; t[1:-1] are filled by rows_dense_eval
        rd = self._rdense = self._dense and T > 2
        full_T, full_sol = T, sol_flat
        if rd:
            if any(not (b > a) for a, b in zip(times, times[1:])):
                raise PnError("-pn_output_times interpolate: the output times must be strictly increasing")
            times_dev = self._rtimes = self.sol_times.to(self.device)
            T, times, sol_flat = 2, [times[0], times[-1]], sol_flat[:: T - 1]
            cols = self._dense_cols
            pv = [v for j in cols for v in list(self._dense_P[j]) + [0.0] * (_lib.PN_DENSE_MAX_POW - len(self._dense_P[j]))]
            P = self._rP = (ctypes.c_double * len(pv))(*pv)
            nxt_out = ops.i32(B)
            nxt_out.fill_(1)                     # times[0] is the initial condition itself
        # the first step of every row: the host engine's own MATCHSTEP clamp at the start of a solve (pn_ts_begin)
        check(lib.pn_ts_begin(ts, 0.0, dt0, T, (ctypes.c_double * T)(*times)))
        t0 = 0.0 if T == 1 else times[0]
        self._rlog, self._rtraj, self._rY = [], ([] if save else None), None
        self._rows_probe = True                    # the first evaluation of this solve is still to come
        self.rounds = 0
        sd, si = ops.f64(4, B), ops.i32(8, B)
        self._rsi = si
        cur = ops.empty(n)
        ops.copy(cur, u0f)
        if T > 1:
            ops.copy(sol_flat[0], u0f)
        if not times[-1] > t0:
            # nothing to integrate (one output time at or before 0; pn_ts_begin has refused a span that does not increase)
            for i in range(T):
                ops.copy(sol_flat[i], u0f)
            si[0].fill_(T)
            self._rows_finish(si[0], si, B, T)
            return solution
        tt, hh = ctypes.c_double(), ctypes.c_double()
        check(lib.pn_ts_attempt(ts, ctypes.byref(tt), ctypes.byref(hh)))
        sd[0].fill_(tt.value)
        sd[1].fill_(hh.value)
        sd[2].fill_(tt.value)
        sd[3].fill_(lib.pn_ts_span_cached_dt(ts))
        if T > 1:
            si[0].fill_(1)                       # times[0] is the initial condition itself
        span = torch.tensor(times, dtype=torch.float64).to(self.device) if T > 1 else None
        nspan = T if T > 1 else 0
        enorm, accept, summary = ops.f64(B), ops.i32(B), ops.i32(4)
        store = save and not self._solution_only and not self._solution_only_auto
        if store:
            self._rY = []
        ie = [j for j in range(s) if e[j] != 0.0 or (not self._fsal and b[j] != 0.0)]
        scratch = [ops.empty(n) for _ in range(s)] if not store else None
        unew_buf = [ops.empty(n), ops.empty(n)]
        pp = [ops.empty(n), cur] if not save else None
        if self._monitor:
            print("round %d: t [%g, %g] dt [%g, %g] rows unfinished %d" % (0, tt.value, tt.value, hh.value, hh.value, B))
        k = 0
        while True:
            if k % _LOG_BLOCK == 0:
                self._rlog.append((ops.f64(_LOG_BLOCK, 3, B), ops.i32(_LOG_BLOCK, B)) + ((ops.i32(_LOG_BLOCK, 2, B),) if rd else ()))
            log_d, log_hit = self._rows_log_at(k)
            h, tr = sd[1], sd[0]
            unew = unew_buf[k % 2]
            Ybuf = [cur] + ([ops.empty(n) for _ in range(1, self._s_eff)] if store else scratch[1:self._s_eff])
            K = [None] * s
            for i in range(s):
                if i == 0:
                    y, targ = cur, sd[2].clone()
                else:
                    y = unew if (self._fsal and i == s - 1) else Ybuf[i]
                    idx = [j for j in range(i) if A[i][j] != 0.0]
                    ops.rows_stage(B, d, y, cur, [K[j] for j in idx], [A[i][j] for j in idx], h)
                    targ = tr + c[i] * h
                K[i] = self._rows_func(self._rows_t(targ), y)
                self.nfe_forward += 1
            ops.rows_combine_wrms(B, d, None if self._fsal else unew, unew if self._fsal else cur, [K[j] for j in ie],
                                  [b[j] for j in ie], [e[j] for j in ie], h, self._atol, self._rtol, enorm)
            ops.rows_control(ts, B, nspan, span, times[-1], enorm, sd, si, log_d, log_hit, accept, summary)
            if save:
                nxt = ops.empty(n)
                self._rtraj.append(cur)
                if store:
                    self._rY.append(Ybuf)
            else:
                nxt = pp[k % 2]
            if rd:
                # the outputs this round's accepted attempts have passed, and the copies of the new state (an exact landing, the
                # final time): log_hit becomes the output copied, as the reverse sweep's masked forcing reads it
                ops.rows_dense_eval(B, d, full_sol, times_dev, cur, [K[j] for j in cols], P, unew, log_d, sd[0], log_hit, nxt_out,
                                    self._rows_range_at(k))
                ops.rows_commit(B, d, nxt, cur, unew, accept, None, None, 0, 0)
            else:
                ops.rows_commit(B, d, nxt, cur, unew, accept, log_hit, sol_flat, n, T)
            cur = nxt
            k += 1
            self.rounds = k
            nopen, frow, fcode = ops.rows_summary(summary)          # the one read-back of the round
            if frow >= 0:
                lib.pn_rows_failure(fcode, frow)
                raise PnError(lib.pn_last_error().decode())
            if self._monitor:
                print("round %d: t [%g, %g] dt [%g, %g] rows unfinished %d"
                      % (k, float(sd[0].min()), float(sd[0].max()), float(sd[1].min()), float(sd[1].max()), nopen))
            if nopen == 0:
                break
        self._rows_finish(nxt_out if rd else si[0], si, B, full_T)
        if self._view:
            print("TS Object (pnode_amd): type rk, -pn_adapt_scope sample: %d rounds for %d rows, accepted steps per row %d..%d, "
                  "rejected %d..%d; output times: %s; launches: %s"
                  % (self.rounds, B, int(self.sample_steps.min()), int(self.sample_steps.max()),
                     int(self.sample_rejections.min()), int(self.sample_rejections.max()),
                     "interpolate (per row, continuous extension of order %d)" % self._dense_order if rd else "match", self._graph_status))
        return solution

    def _rows_finish(self, served, si, B, T):
        """`served`: per row, the number of output times it has reached (the span counter, or the rows' own counter)."""
        host = si.cpu()
        self.sample_steps = host[1].clone()
        self.sample_rejections = host[2].clone()
        self._nsteps = int(self.sample_steps.max()) if B else 0
        if T > 1:
            short = (served.cpu() != T).nonzero()
            if short.numel():
                raise Exception("TSSolve fails to step on all the specified points (-pn_adapt_scope sample: row %d)" % int(short[0]))

    # ------------------------------------------------------------------ reverse rounds
    def _rows_reverse(self, g, T):
        """The exact discrete adjoint of the logged per-row step sequences (step sizes held constant): the rounds in reverse,
        row r of round k with the logged h_eff[k][r]."""
        if self._rtraj is None:
            raise RuntimeError("adjoint requested but no trajectory was saved "
                               "(setupTS(enable_adjoint=True) and a differentiable input are required)")
        ops = self._ops
        B, n = self._rB, self.n
        d = n // B
        s_eff, A, b, c = self._s_eff, self._A, self._b, self._c
        rd = self._rdense
        # the stages of a reversed round.  With interpolated outputs whose extension uses the last stage of a first-same-as-last
        # tableau, that stage is an ordinary one here (nothing is routed between rounds: stage 0 is re-evaluated every round):
        # Y_{s-1} = u + h sum_j a_{s-1,j} K_j, cotangent D_{s-1} alone -- one more evaluation and VJP per reversed round
        stages = list(range(s_eff))
        if rd and self._fsal and (self._s - 1) in self._dense_cols:
            stages.append(self._s - 1)
        lam = self.adj_u_tensor = self.adj_u_flat = ops.empty(n)
        lam.zero_()
        if self.adj_p_tensor is None or self.adj_p_tensor.numel() != self.np:
            self.adj_p_tensor = ops.empty(max(self.np, 1))[: self.np]
        self.adj_p_tensor.zero_()
        self._pend_a, self._pend_g = [], []
        self._pend_mixed = False
        self._pend_bias, self._pend_bias_bytes = [], 0
        g = g.contiguous()
        ld = g.stride(0)
        R = self.rounds
        if R == 0:
            ops.rows_adj_accum(B, d, lam, lam, [], g, ld, ops.i32(B), T)
            return
        hit0 = ops.i32(B) if T > 1 else None           # every row's state at t[0] is u0
        ops.rows_adj_accum(B, d, lam, lam, [], g, ld, self._rows_log_at(R - 1)[1], T)
        wbuf = ops.empty(n)
        ybuf = [None] + [ops.empty(n) for _ in range(1, stages[-1] + 1)]
        if rd:
            cols = self._dense_cols
            Dbuf = dict((j, ops.empty(n)) for j in cols)
            Gbuf = ops.empty(n)
        for k in range(R - 1, -1, -1):
            log_d, _ = self._rows_log_at(k)
            heff, tr, tf = log_d[0], log_d[1], log_d[2]
            u = self._rtraj[k]
            Y = self._rY[k] if self._rY is not None else None
            tapes, K = {}, {}
            for i in stages:
                if i == 0:
                    y, targ = u, tf.clone()
                else:
                    if Y is not None and i < s_eff:
                        y = Y[i]
                    else:
                        y = ybuf[i]
                        idx = [j for j in range(i) if A[i][j] != 0.0]
                        ops.rows_stage(B, d, y, u, [K[j] for j in idx], [A[i][j] for j in idx], heff)
                    targ = tr + c[i] * heff
                rec = []
                K[i] = self._rows_func(self._rows_t(targ), y, rec)
                tapes[i] = rec[0]
                self.nfe_backward += 1
            if rd:
                # D_j[r] = sum_o h_r beta_j(theta_o) g[o, r] over the outputs row r interpolated in this round, G[r] = sum_o g[o, r]
                ops.rows_dense_adjoint(B, d, [Dbuf[j] for j in cols], Gbuf, g, self._rtimes, self._rP, self._rows_range_at(k), log_d)
            dlam = [None] * self._s
            for i in reversed(stages):
                js = [j for j in stages if j > i and A[j][i] != 0.0 and dlam[j] is not None]
                Di = Dbuf.get(i) if rd else None
                if b[i] == 0.0 and not js and Di is None:
                    continue
                if b[i] == 0.0 and not js:
                    w = Di                               # the stage's cotangent is what its outputs send it
                else:
                    w = wbuf
                    if Di is None:
                        ops.rows_adj_theta(B, d, w, lam if b[i] != 0.0 else None, b[i], [dlam[j] for j in js], [A[j][i] for j in js], heff)
                    else:
                        ops.rows_adj_theta(B, d, w, lam if b[i] != 0.0 else None, b[i], [dlam[j] for j in js], [A[j][i] for j in js], heff,
                                           dense_w=Di)
                y, out, wrt = tapes[i]
                tapes[i] = None
                grads = torch.autograd.grad(out, (y,) + tuple(wrt), self._shaped(w).view(out.shape), allow_unused=True)
                gy = grads[0]
                if gy is not None:
                    if gy.dtype != self.tensor_dtype:
                        gy = gy.to(self.tensor_dtype)
                    gy = gy.contiguous().reshape(-1)
                    if gy.untyped_storage().data_ptr() == w.untyped_storage().data_ptr():
                        gy = gy.clone()
                dlam[i] = gy
                wst = w.untyped_storage().data_ptr()
                gp = []
                for q in grads[1:]:
                    if q is not None:
                        if q.dtype != self.tensor_dtype or not q.is_contiguous():
                            q = q.to(self.tensor_dtype).contiguous()
                        if q.untyped_storage().data_ptr() == wst:
                            q = q.clone()
                    gp.append(q)
                if self.np > 0 and any(q is not None for q in gp):
                    self._pend_a.append(1.0)              # the row's h is inside the cotangent
                    self._pend_g.append(gp)
            self._flush_param_accum()
            terms = [dlam[i] for i in stages if dlam[i] is not None]
            if rd:
                terms.append(Gbuf)
            if len(terms) > _lib.PN_MAX_STAGES:          # (5dp with interpolated outputs: seven stages and G)
                ops.rows_adj_accum(B, d, lam, lam, terms[_lib.PN_MAX_STAGES:], None, ld, None, T)
                terms = terms[: _lib.PN_MAX_STAGES]
            hit_prev = self._rows_log_at(k - 1)[1] if k > 0 else hit0
            ops.rows_adj_accum(B, d, lam, lam, terms, g if hit_prev is not None else None, ld, hit_prev, T)
            self._rtraj[k] = None
            if self._rY is not None:
                self._rY[k] = None
        self._flush_param_accum()

