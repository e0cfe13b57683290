"""The explicit Runge-Kutta sweeps behind ``ODEPetsc`` (pnode_amd/petsc_adjoint.py, the reference-shaped surface), as a mixin: what
PETSc's ``TSSolve`` / ``TSStep_RK`` / ``TSAdjointStep_RK`` / ``TSTrajectoryGet`` do between two callbacks into Python (SURVEY 8a-3, a-6,
a-8, a-9, a-10), forward beside reverse.  The callback shells and the step; the forward sweep (begin / accepted step / end; dense output,
time span, trajectory and tape policy); the step advance both directions share; recomputation from checkpoints; the reverse sweep, dL/dt."""
import contextlib
import ctypes
import warnings

import torch

from . import _lib, options
from ._lib import PnError, check  # noqa: F401


def _mem_now(device):
    """(bytes allocated, bytes reserved) by PyTorch's caching allocator on `device`.  torch.cuda.memory_allocated()
    flattens the whole statistics dictionary in Python (~90 us per call, measured in the eager sweep's profile); the
    nested dictionary underneath costs a tenth of that."""
    try:
        st = torch._C._cuda_memoryStats(device.index if device.index is not None else torch.cuda.current_device())
        return st["allocated_bytes"]["all"]["current"], st["reserved_bytes"]["all"]["current"]
    except Exception:
        return torch.cuda.memory_allocated(device), torch.cuda.memory_reserved(device)


class _RKState(object):
    """The state of one forward sweep (RKSweep._rk_begin); slots: the step loop reads and writes it once per accepted step."""
    __slots__ = "save T times full solution sol traj keep_tape tape_budget tape_steps tape_fsal K_fsal pingpong pp cur cur_slot ctl finished".split()


class RKSweep(object):
    def _func_with_grad(self, t, y, which="EX"):
        """f(t, y) recorded by autograd; returns (output, parameter tensors to differentiate
        with respect to).  While a hipGraph is being captured the parameters are replaced by
        fresh detached aliases (same storage): the real parameters' AccumulateGrad nodes live
        on the stream of the enclosing autograd graph and a gradient edge to them would make
        autograd synchronise the capture stream with that stream."""
        fn, params, names = ((self.funcIM, self._paramsI, self._pnamesI) if which == "IM"
                             else (self.funcEX, self._paramsE, self._pnamesE))
        lin = self._lin if (which == "EX" and self._lin is not None and self._lin.active) else None
        capturing = self.device.type == "cuda" and params and torch.cuda.is_current_stream_capturing()
        seen = tuple(p.detach().requires_grad_(True) for p in params) if capturing else params
        if lin is not None:
            lin.begin()                # func's Linear layers hook their outputs: dW / db are accumulated by the engine
        fwd = self._fwd if (which == "EX" and self._fwd is not None and self._fwd.active) else None
        out = None
        try:
            # (the window: eligible Linear -> Tanh pairs of func run as one launch each, pnode_amd/_linearfwd.py)
            with (fwd.window(lin) if fwd is not None else contextlib.nullcontext()):
                if capturing:
                    out = torch.func.functional_call(fn, dict(zip(names, seen)), (t, y))
                else:
                    out = fn(t, y)
        finally:
            if lin is not None and out is None:
                lin.abort()
        # the structural check of THIS evaluation (pnode_amd/_lineargrad.py): a handled weight or bias that func also used
        # outside its layer's call leaves the whole evaluation to autograd, as the reference does with every evaluation
        if lin is None or not lin.end(out, [seen[k] for k in lin.handled]):
            return out, seen
        return out, tuple(seen[k] for k in lin.rest)

    def _call_func(self, t, y_flat, tape=None, slot=None):
        """evalRHSFunction (pa.py:393-412): K = f(t, Y); no copy of the result.  With `tape`
        (a list) the evaluation is recorded by autograd and (input, output) is appended.  `slot`: the stage index, given by
        the callers whose evaluations an adaptive sweep replays from per-evaluation hipGraphs (pnode_amd/_stagegraphs.py)."""
        if slot is not None and self._sg is not None:
            return self._sg.evaluate(self, slot, t, y_flat, tape)
        y = self._shaped(y_flat)
        if self._tgrad:
            t = self._t_arg(t, tape is not None)      # (every evaluation of such a solve: forward and adjoint see the same f)
        if tape is not None:
            with torch.enable_grad():
                y = y.detach().requires_grad_(True)
                k, wrt = self._func_with_grad(t, y)
            tape.append((y, k, wrt, t) if self._tgrad else (y, k, wrt))
        elif self._fwd is not None and self._fwd.active:
            with self._fwd.window():
                k = self.funcEX(t, y)
        else:
            k = self.funcEX(t, y)
        k = self._func_result(k, y_flat)
        self.nfe_forward += 1
        return k

    def _func_result(self, k, y_flat, numel=None):
        """func's result as both sweeps take it: refused unless it has the state's shape, dtype and device; flat, detached,
        contiguous, and a copy when func returned (a view of) its input -- the input buffer is recycled.  `numel`: the entries
        of the state func was called with, where that is a part of the batch (-pn_rows_compact 1)."""
        if k.dtype != self.tensor_dtype or k.device != self.device or k.numel() != (self.n if numel is None else numel):
            raise ValueError("func must return a tensor with the state's shape, dtype and device")
        k = k.detach()
        if not k.is_contiguous():
            k = k.contiguous()
        if k.untyped_storage().data_ptr() == y_flat.untyped_storage().data_ptr():
            k = k.clone()
        return k.reshape(-1)

    def _rk_step(self, t, h, u, K0, unew, stage_dest, want_err, tapes=None, t_first=None):
        """One explicit RK step attempt from the flat state `u` (TSStep_RK's body).

        `t_first`: time at which the first stage derivative is evaluated when it is not handed in
        (see `_first_stage_time`).

        stage_dest(i) -> flat buffer for stage value Y_i, 1 <= i < s (FSAL: Y_{s-1} is `unew`).
        Returns the stage derivatives K (K[s-1] is the FSAL derivative of the next step).
        `tapes` (list of s entries, filled here) receives the autograd tape of each stage.
        """
        ops, s, A, b = self._ops, self._s, self._A, self._b
        if self._native and not (want_err and self._vtol is not None):
            # (per-component tolerances do not fit pn_vec_ops.rk_combine_wrms, which carries two scalars: such an attempt takes the
            # stage loop below -- the same launches, the same bits -- and ends in the _v form of the norm, _errnorm.py)
            return self._rk_step_native(t, h, u, K0, unew, stage_dest, want_err, tapes, t_first)
        plan = self._stage_plan(h)
        K = [None] * s
        for i in range(s):
            if i == 0:
                y = u
            else:
                y = unew if (self._fsal and i == s - 1) else stage_dest(i)
                idx, coef = plan[i]
                ops.rk_stage(y, u, [K[j] for j in idx], coef)
            if i == 0 and K0 is not None:
                K[0] = K0
            elif tapes is not None:
                rec = []
                K[i] = self._call_func(t + self._c[i] * h, y, rec, slot=i)
                tapes[i] = rec[0]
            else:
                K[i] = self._call_func(t_first if (i == 0 and t_first is not None) else t + self._c[i] * h, y, slot=i)
        if want_err:
            idx = [j for j in range(s) if self._e[j] != 0.0 or (not self._fsal and b[j] != 0.0)]
            self._err_combine(None if self._fsal else unew, unew if self._fsal else u, [K[j] for j in idx],
                              [h * b[j] for j in idx], [h * self._e[j] for j in idx])
        elif not self._fsal:
            idx, coef = plan[s]
            ops.rk_stage(unew, u, [K[j] for j in idx], coef)
        return K

    # ---- the C++ step loops (include/pnode_amd.h section 3a) and their two callbacks
    def _make_callbacks(self):
        import weakref
        ref = weakref.ref(self)

        def stage_cb(user, i, t):
            o = ref()
            try:
                tens, tapes, K = o._cbs
                if tapes is not None:
                    rec = []
                    k = o._call_func(t, tens[i], rec, slot=i)
                    tapes[i] = rec[0]
                else:
                    k = o._call_func(t, tens[i], slot=i)
                K[i] = k                                # keeps the derivative alive; the loop gets its address
                return k.data_ptr()
            except BaseException as exc:                # (an exception must not propagate through the C frame)
                o._cb_exc = exc
                return 0

        def vjp_cb(user, i, t, cot_in_w, scale):
            o = ref()
            try:
                Y, tapes, dlam, t0 = o._rcbs
                if i == 0 and t0 is not None:
                    t = t0                              # first-same-as-last: where the forward sweep evaluated this stage
                w = o.adj_u_flat if not cot_in_w else o._buf("w_a" if cot_in_w == 1 else "w_b")
                gy, gp = o._vjp(t, Y[i], w, tapes[i] if tapes else None, alpha=scale, last=(i == 0), slot=i)
                if tapes:
                    tapes[i] = None                     # release the stage's activations as soon as they are used
                if gy is not None and gy.data_ptr() == w.data_ptr():
                    gy = gy.clone()                     # f returned its cotangent unchanged (identity-like f)
                dlam[i] = gy
                o._take_param_grads(scale, gp, deferred=o._accum_mode != "stage")
                return 0 if gy is None else gy.data_ptr()
            except BaseException as exc:
                o._cb_exc = exc
                return -1

        self._stage_cb_c = _lib.STAGE_CB(stage_cb)
        self._vjp_cb_c = _lib.VJP_CB(vjp_cb)
        self._ystage = (ctypes.c_void_p * _lib.PN_MAX_STAGES)()
        self._kout = (ctypes.c_void_p * _lib.PN_MAX_STAGES)()
        self._ytens = [None] * _lib.PN_MAX_STAGES
        self._cb_exc = None

    def _raise_from_loop(self, rc):
        exc, self._cb_exc = self._cb_exc, None
        if exc is not None:
            raise exc
        check(rc)

    def _rk_step_native(self, t, h, u, K0, unew, stage_dest, want_err, tapes, t_first):
        ops, s = self._ops, self._s
        if getattr(self, "_stage_cb_c", None) is None:
            self._make_callbacks()
        ys, tens = self._ystage, self._ytens
        tens[0] = u
        for i in range(1, s):
            y = unew if (self._fsal and i == s - 1) else stage_dest(i)
            tens[i] = y
            ys[i] = y.data_ptr()
        K = [None] * s
        K[0] = K0
        self._cbs = (tens, tapes, K)
        work, res = ops.wrms_buffers() if want_err else (None, None)
        rc = self._lib.pn_rk_attempt(ops.stream(), ops.code, self.n, self._ts, self._err_vec_ops(), t, h, u.data_ptr(), unew.data_ptr(), ys,
                                     None if K0 is None else K0.data_ptr(),
                                     1 if (K0 is None and t_first is not None) else 0, 0.0 if t_first is None else t_first,
                                     self._stage_cb_c, None, 1 if want_err else 0, work, res, self._kout)
        self._cbs = None
        if rc:
            self._raise_from_loop(rc)
        return K

    def _stage_plan(self, h):
        """Per stage i: (indices j of the non-zero a_ij, the coefficients h*a_ij as a C array); entry s: the same for
        the weights b.  Built once per step size (fixed-step sweeps use one; adaptive ones a few dozen)."""
        plan = self._plans.get(h)
        if plan is None:
            if len(self._plans) >= 256:
                self._plans.clear()
            mk = getattr(self._ops, "dbl", list)
            s, A, b = self._s, self._A, self._b
            plan = []
            for i in range(s):
                idx = [j for j in range(i) if A[i][j] != 0.0]
                plan.append((idx, mk([h * A[i][j] for j in idx])))
            idx = [j for j in range(s) if b[j] != 0.0]
            plan.append((idx, mk([h * b[j] for j in idx])))
            self._plans[h] = plan
        return plan

    # ------------------------------------------------------------------ forward sweep (pa.py:777-869)
    def _rk_odeint(self, u0, t, save):
        """ts.solve (pa.py:829) for the explicit RK tableaus with one step-size controller for the whole batch."""
        st = self._rk_begin(u0, t, save)
        while not self._rk_accept_step(st):
            pass
        return self._rk_end(st)

    def _rk_begin(self, u0, t, save):
        """The state of a forward sweep: the span as the stepper sees it, the trajectory and the tape policy (_rk_trajectory), the
        ping-pong pair for states no checkpoint holds, and the initial state in its home."""
        lib, ops, ts = self._lib, self._ops, self._ts
        self.sol_times = t.detach().cpu().to(dtype=torch.float64)
        T, times = int(t.shape[0]), self.sol_times.tolist()
        dt0 = float(self.step_size[0] if isinstance(self.step_size, list) else self.step_size)
        st = _RKState()
        st.save, st.T, st.times, st.full, st.K_fsal, st.tape_fsal, st.tape_steps = save, T, times, None, None, None, 0
        st.solution = ops.empty((T,) + tuple(self.tensor_size))
        st.sol = st.solution.view(T, -1)
        # -pn_output_times interpolate: the stepper sees the end points only; t[1:-1] are filled by _dense_step
        self._dense_active = self._dense and T > 2
        if self._dense_active:
            if any(not (b > a) for a, b in zip(times, times[1:])):
                raise PnError("-pn_output_times interpolate: the output times must be strictly increasing")
            st.full = (T, times, st.sol)
            st.T, st.times, st.sol = 2, [times[0], times[-1]], st.sol[:: T - 1]      # rows 0 and T-1 of the solution
            self._dense_next = 1
        T, times = st.T, st.times
        check(lib.pn_ts_begin(ts, 0.0, dt0, T, (ctypes.c_double * T)(*times)))
        self._span_begin(T)
        u0f = u0.detach().contiguous().reshape(-1)
        self._rk_trajectory(st)
        st.pingpong, st.pp = [self._buf("u_a"), self._buf("u_b")], 0
        st.cur, st.cur_slot = self._state_home(st, 0)
        ops.copy(st.cur[0], u0f)
        if T > 1:
            ops.copy(st.sol[0], u0f)
        st.ctl = (ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(0))   # t_n, h, accepted, hit, done
        st.finished = not (times[-1] > (0.0 if T == 1 else times[0]))
        if self._monitor:
            print("%d TS dt %g time %g" % (0, dt0, 0.0 if T == 1 else times[0]))
        return st

    def _rk_trajectory(self, st):
        """Where the state at the start of every step will live (the solve was just begun, pn_ts_begin done), and whether
        the stages' autograd tapes are kept for the reverse sweep."""
        self._tmode = self._pick_traj_mode(self._s_eff) if st.save else self._traj_mode
        st.traj = self._traj = None
        if st.save:
            vecs = self._s_eff if (self._tmode == _lib.PN_TRAJ_ALL or self._budget_stages) else 1
            st.traj = self._traj = self._new_trajectory(vecs, self._tmode)
            if self._tmode == _lib.PN_TRAJ_BUDGET and not self._adaptive and not isinstance(self.step_size, list):
                total = self._lib.pn_ts_count_fixed_steps(self._ts)         # fixed step: the sweep length is known
                if total > 0:
                    check(self._lib.pn_traj_set_total(st.traj.handle, total))
        # (per-evaluation graphs, pnode_amd/_stagegraphs.py: a captured evaluation's tape is overwritten by its next replay)
        st.keep_tape = st.save and self._tmode == _lib.PN_TRAJ_ALL and self._retain_graph != 0 and self._sg is None
        st.tape_budget = None
        if st.keep_tape and self._retain_graph == 2:
            st.tape_budget = self._tape_budget()
            st.keep_tape = st.tape_budget is not None and st.tape_budget > 0
        self._tapes = {} if st.keep_tape else None

    def _state_home(self, st, step):
        """(view, slot) of the state at the start of `step`: its trajectory slot's (vecs, npad), or a ping-pong buffer's (1, npad) and -1."""
        traj = st.traj
        if traj is not None:
            slot = traj.fwd_slot(step)
            if slot >= 0:
                traj.stage_step.pop(slot, None)  # a recycled slot no longer holds the old step's stages
                return traj.claim(slot), slot
        st.pp ^= 1
        return st.pingpong[st.pp].view(1, -1), -1

    def _rk_advance(self, cur, cur_slot, nxt, tn, h, K0, want_err, tapes=None, t_first=None):
        """One attempt of the step [tn, tn+h] from the state in the view `cur` (of trajectory slot `cur_slot`, -1: none) into the
        view `nxt`, in either direction of the sweep: the stage values go behind the checkpoint `cur` lives in where the
        trajectory keeps them, else into scratch.  Returns the stage derivatives K (see _rk_step)."""
        kept = cur_slot >= 0 and (self._tmode == _lib.PN_TRAJ_ALL or self._budget_stages)
        dest = (lambda i: cur[i]) if kept else (lambda i: self._buf("y_scratch"))
        return self._rk_step(tn, h, cur[0], K0, nxt[0], dest, want_err, tapes, t_first)

    def _rk_step_stands(self, k, cur_slot, K, state_sealed):
        """Step k, advanced by _rk_advance from trajectory slot `cur_slot` (-1: none), stands (a rejected forward attempt must not seal):
        the slot carries the step's stage values now, if budgeted checkpoints keep them, and is complete.  `state_sealed`: a re-advance
        starts from complete checkpoints, the forward sweep seals once, here.  Returns K_0 of step k+1 for a first-same-as-last tableau."""
        if cur_slot >= 0:
            if self._budget_stages:
                self._traj.stage_step[cur_slot] = k
            if self._budget_stages or not state_sealed:
                self._traj.seal(cur_slot)          # (a no-op on the HBM tier)
        return K[self._s - 1] if self._fsal else None

    def _rk_accept_step(self, st):
        """One accepted step of the forward sweep: attempts until pn_ts_judge accepts one, then what follows an accepted step.
        Returns whether the solve is finished."""
        if st.finished:
            return True                  # (an empty span: nothing to step over)
        lib, ts, s, adaptive = self._lib, self._ts, self._s, self._adaptive
        tt, hh, acc, hit, done = st.ctl
        cur, cur_slot, keep_tape = st.cur, st.cur_slot, st.keep_tape
        step = lib.pn_ts_steps(ts)
        nxt, nxt_slot = self._state_home(st, step + 1)
        K0, tape0 = st.K_fsal, st.tape_fsal
        while True:
            check(lib.pn_ts_attempt(ts, ctypes.byref(tt), ctypes.byref(hh)))
            tn, h = tt.value, hh.value
            tapes = [tape0] + [None] * (s - 1) if keep_tape else None
            K = self._rk_advance(cur, cur_slot, nxt, tn, h, K0, adaptive, tapes)
            if keep_tape:
                tape0 = tapes[0]
            enorm = self._global_enorm(self._err_read()) if adaptive else -1.0
            check(lib.pn_ts_judge(ts, enorm, ctypes.byref(acc), ctypes.byref(hit), ctypes.byref(done)))
            if acc.value:
                break
            K0 = K[0]            # f(t_n, u_n) does not depend on h
        if keep_tape:
            self._rk_keep_tapes(st, step, tapes)
        st.K_fsal = self._rk_step_stands(step, cur_slot, K, False)
        st.cur, st.cur_slot = nxt, nxt_slot
        tnew = lib.pn_ts_time(ts)
        self._span_post_step(st.T, st.times, hit.value, done.value, step + 1, tnew, nxt[0], st.sol)
        if st.full is not None:
            self._dense_step(tn, h, tnew, cur[0], K, nxt[0], st.full[1], st.full[2])
        if self._monitor:
            print("%d TS dt %g time %g" % (step + 1, h, tnew))
        st.finished = bool(done.value)
        return st.finished

    def _rk_keep_tapes(self, st, step, tapes):
        """The accepted step's tapes go to the reverse sweep; in `auto` mode, as long as the budget measured at step 0 lasts."""
        self._tapes[step] = tapes[: self._s_eff]
        st.tape_fsal = tapes[self._s - 1] if self._fsal else None
        if st.tape_budget is not None and st.tape_budget != float("inf"):
            if step == 0:                 # one measurement: what a step's tapes (and its slot) take
                per_step = max(_mem_now(self.device)[0] - self._tape_mem0, 1)
                st.tape_steps = int(st.tape_budget // per_step) - 1
            if step + 1 >= st.tape_steps:
                st.keep_tape, st.tape_fsal = False, None       # later steps re-evaluate f in the reverse sweep
                self._tape_all_fit = False

    def _rk_end(self, st):
        """The closing bookkeeping of a forward sweep: -ts_view, the T == 1 copy, the span and dense end checks; returns the solution."""
        self._nsteps = self._lib.pn_ts_steps(self._ts)
        if self._view:
            self._ts_view()
        if st.T == 1:
            self._ops.copy(st.sol[0], st.cur[0])
        else:
            self._span_end(st.T)
        if st.full is not None:
            if self._dense_next != st.full[0] - 1:
                raise Exception("TSSolve fails to step on all the specified points")
            if st.save and self._fsal:
                self._ops.copy(self._buf("dense_yN"), st.cur[0])       # where the last step's FSAL derivative was evaluated (reverse sweep)
        return st.solution

    # ------------------------------------------------------------------ dense output (-pn_output_times interpolate)
    def _dense_coefs(self, to, tn, h):
        """h*beta_j(theta) for every stage j, theta = (to - tn)/h, in double (rounded once to the storage type by the kernels)."""
        th = (to - tn) / h
        out = []
        for row in self._dense_P:
            v = 0.0
            for p in reversed(row):
                v = (v + p) * th
            out.append(h * v)
        return out

    def _dense_step(self, tn, h, tnew, u, K, unew, times, sol):
        """After the accepted step [tn, tnew] (stage derivatives K, start state u, end state unew): the output times inside it
        from the continuous extension in ONE launch, an output time equal to tnew as a copy of the state."""
        T = len(times)
        lo = o = self._dense_next
        while o < T - 1 and times[o] < tnew:
            o += 1
        if o > lo:
            cols = self._dense_cols
            coefs = []
            for q in range(lo, o):
                c = self._dense_coefs(times[q], tn, h)
                coefs.append([c[j] for j in cols])
            self._ops.dense_eval(sol[lo:o], u, [K[j] for j in cols], coefs)
        if o < T - 1 and times[o] == tnew:
            self._ops.copy(sol[o], unew)
            o += 1
        self._dense_next = o

    # ------------------------------------------------------------------ time span (pa.py:518-532, 822-868)
    def _span_begin(self, T):
        self.cur_sol_steps = [0] * T      # steps taken from the previous output time to this one
        self.cur_sol_index = 1
        self._span_hits = 1               # output times whose solution has been kept (t[0] is u0)
        self._span_delta = 1e-5 if self.tensor_dtype == torch.double else 1e-3

    def _span_post_step(self, T, times, hit, done, stepno, tnew, cur, sol_flat):
        """What happens after an accepted step of a multi-output solve.

        * The output itself: the reference reads PETSc's ``getTimeSpanSolutions()`` (pa.py:845), i.e.
          the state of exactly the step that landed on t[i].  Here: ``pn_ts_judge`` reports that step
          (`hit` = i) and the state is copied out then.
        * ``tspanPostStep`` (pa.py:518-532): a ``step_size`` list sets the next step; the steps of
          each output interval are counted for the reverse sweep.  The reference advances its
          interval counter when ``|t - t[i]| < 1e-5`` (fp64) / ``1e-3`` (fp32), which is one step
          early whenever the step is shorter than that window: its backward pass then injects
          dL/dy(t[i]) one step off and never reverses the sweep's first step.  The default here
          counts with the exact hit (the discrete adjoint of what the forward sweep computed);
          ``-pn_span_count reference`` counts as the reference does (identical whenever every step
          is longer than the window)."""
        if T <= 1:
            return
        if hit >= 0:
            self._ops.copy(sol_flat[hit], cur)
            self._span_hits += 1
        if self.cur_sol_index < T:
            if isinstance(self.step_size, list) and stepno < len(self.step_size) and not done:
                check(self._lib.pn_ts_override_next_dt(self._ts, float(self.step_size[stepno])))
            self.cur_sol_steps[self.cur_sol_index] += 1
            if self._span_count_reference:
                if abs(tnew - times[self.cur_sol_index]) < self._span_delta:
                    self.cur_sol_index += 1
            elif hit >= 0:
                self.cur_sol_index = hit + 1

    def _span_end(self, T):
        if self.cur_sol_index != T or self._span_hits != T:
            raise Exception("TSSolve fails to step on all the specified points")

    def _pick_traj_mode(self, vecs_all):
        """Trajectory mode of the solve that was just begun (pn_ts_begin done).  When
        -ts_trajectory_solution_only is not given PETSc keeps the states only and recomputes a step's
        stages when it is reversed.  Every mode replays the same arithmetic -- gradients are identical bit
        for bit -- so on a 288 GB part the stage values are kept as well whenever the step count is known
        (fixed step) and the whole trajectory fits in a quarter of the HBM that is free right now: the
        reverse sweep then recomputes nothing.  Give the option (0 or 1) to decide yourself."""
        mode = self._traj_mode
        if (mode != _lib.PN_TRAJ_SOLUTION or not self._solution_only_auto or self.device.type != "cuda"
                or isinstance(self.step_size, list)):
            return mode
        if torch.cuda.is_current_stream_capturing():        # no driver query while capturing: as the last eager solve
            return getattr(self, "_tmode_auto", mode)
        total = self._lib.pn_ts_count_fixed_steps(self._ts)
        self._tmode_auto = mode
        if total > 0:
            esize = 4 if self.tensor_dtype == torch.float32 else 8
            need = (total + 1) * vecs_all * self._npad * esize
            free, _ = torch.cuda.mem_get_info(self.device)
            allocated, reserved = _mem_now(self.device)
            if need <= 0.25 * (free + max(reserved - allocated, 0)):
                self._tmode_auto = _lib.PN_TRAJ_ALL
        return self._tmode_auto

    def _tape_budget(self):
        """Bytes the retained tapes of this sweep may take in `auto` mode: half of the HBM that is free now
        (driver-free + cached-but-unused blocks of PyTorch's allocator); None on the CPU test stand-in.
        While a hipGraph is being captured no driver query is made: the sweep keeps what the eager
        warm-up call before it kept."""
        if self.device.type != "cuda":
            return None
        if torch.cuda.is_current_stream_capturing():
            return float("inf") if getattr(self, "_tape_all_fit", False) else None
        self._tape_mem0, reserved = _mem_now(self.device)
        free, _ = torch.cuda.mem_get_info(self.device)
        self._tape_all_fit = True
        return 0.5 * (free + max(reserved - self._tape_mem0, 0))

    def _first_stage_time(self, k):
        """Time argument of f for the first stage of step k when it is RE-computed from a checkpoint.
        In the original sweep of a first-same-as-last tableau that derivative was the previous step's
        last stage, evaluated at t_{k-1} + c_{s-1} h_{k-1}; that is not t_k to the last bit (5dp's
        c_{s-1} is the row sum 0.9999999999999998; matched output times are set exactly), and a
        time-dependent f would see it.  Same expression here, so that every checkpoint mode
        reproduces the store-all sweep bit for bit."""
        if self._fsal and k > 0 and not self._ref_defaults:
            tp, hp = self._step_info(k - 1)
            return tp + self._c[self._s - 1] * hp
        # (-pn_reference_defaults: PETSc's TSTrajectory restarts the stepper at a restored checkpoint, so the first stage is
        # re-evaluated -- and its Jacobian taken, TSAdjointStep_RK -- at t_k; for a time-dependent f under a first-same-as-last
        # tableau that is the forward sweep's derivative only up to the last bits of the time argument, as with the reference)
        return None

    def _stages_of(self, step):
        """Stage values Y_0..Y_{s_eff-1} of `step` as flat tensors: read from the store-all
        trajectory, or recomputed from the nearest kept state (TSTrajectoryGet)."""
        traj = self._traj
        fs, fl, stores = traj.rev_plan(step)
        if self._tmode == _lib.PN_TRAJ_ALL or (self._budget_stages and fs == step and traj.stage_step.get(fl) == step):
            v = traj.view(fl)              # (budgeted checkpoints: the checkpoint of this very step holds its stage values)
            return [v[i] for i in range(self._s_eff)]
        return self._stage_values(step, *self._readvance(fs, fl, stores, step))

    def _readvance(self, fs, fl, stores, step):
        """Re-advance from the checkpoint of step `fs` in slot `fl` to the start of `step`, keeping what the plan asks for
        (`stores`: step -> slot of a new checkpoint).  Returns (flat state at the start of `step`, its K_0 or None)."""
        traj, keep = self._traj, self._budget_stages
        cur, cur_slot = traj.view(fl), fl
        K_fsal, pp = None, 0
        for k in range(fs, step):
            tn, h = self._step_info(k)
            nxt_slot = stores.get(k + 1, -1)
            if nxt_slot >= 0:
                nxt = traj.claim(nxt_slot)
                traj.stage_step.pop(nxt_slot, None)
            else:
                pp ^= 1
                nxt = self._buf("r_a" if pp else "r_b").view(1, -1)
            K = self._rk_advance(cur, cur_slot, nxt, tn, h, K_fsal, False,
                                 t_first=self._first_stage_time(k) if K_fsal is None else None)
            K_fsal = self._rk_step_stands(k, cur_slot, K, True)
            if nxt_slot >= 0 and not keep:
                traj.seal(nxt_slot)                  # (disk tier) a new state-only checkpoint is complete
            cur, cur_slot = nxt, nxt_slot
        return cur[0], K_fsal

    def _stage_values(self, step, cur, K_fsal):
        """Stage values of `step` itself from its start state `cur` (its own derivatives K_0..K_{s_eff-2} are needed)."""
        ops, s_eff = self._ops, self._s_eff
        tn, h = self._step_info(step)
        plan = self._stage_plan(h)
        Y, K = [cur], [K_fsal]
        # The derivatives K_0..K_{s_eff-2} evaluated here are evaluations of f at exactly the points the stage VJPs of this
        # step differentiate f at: unless tapes are switched off (-pn_trajectory_retain_graph 0, -pn_reference_defaults) they
        # are recorded by autograd and the VJPs of those stages run their backward half only -- (s_eff - 1) evaluations of f
        # fewer per reversed step in every mode that recomputes stage values (solution-only, checkpoint budgets); same bits.
        rt = [None] * self._s if self._retain_graph != 0 else None
        self._rtapes = rt
        for i in range(1, s_eff):
            if K[i - 1] is None:
                t_eval = self._first_stage_time(step) if i == 1 else None
                tt = tn + self._c[i - 1] * h if t_eval is None else t_eval
                rec = [] if rt is not None else None
                K[i - 1] = self._call_func(tt, Y[i - 1], rec, slot=i - 1)
                if rt is not None:
                    rt[i - 1] = rec[0]
            y = self._buf("ys%d" % i)
            ops.rk_stage(y, cur, [K[j] for j in plan[i][0]], plan[i][1])
            Y.append(y)
            K.append(None)
        if self._ref_defaults:
            # -pn_reference_defaults: PETSc's TSTrajectory re-runs the WHOLE step (TSStep) to get the stage values back,
            # i.e. it also evaluates the stage derivatives nothing in the reverse sweep reads.  Evaluated here too (and
            # dropped), so that a func that counts its calls sees s evaluations per recomputed step.
            if K[s_eff - 1] is None:
                K[s_eff - 1] = self._call_func(tn + self._c[s_eff - 1] * h, Y[s_eff - 1])
            if self._fsal:
                i = self._s - 1
                y = self._buf("y_scratch")
                ops.rk_stage(y, cur, [K[j] for j in plan[i][0]], plan[i][1])
                self._call_func(tn + self._c[i] * h, y)
        return Y

    def _vjp(self, t, y_flat, w_flat, tape=None, which="EX", alpha=None, last=False, slot=None):
        """RHSJacShell.multTranspose + RHSJacPShell.multTranspose (pa.py:52-82, 341-363): one
        forward of f with grad and one backward with the cotangent `w`; returns
        (J^T w as a flat tensor or None, list of parameter cotangents over ALL parameters of that f).  With a `tape`
        (input, output) recorded in the forward sweep only the backward runs.  `alpha`: the scale the caller will give the
        parameter cotangents when it adds them to mu -- the explicit RK path passes it so that the sensitivities of func's
        nn.Linear layers can be accumulated during the backward pass itself (pnode_amd/_lineargrad.py); those entries of
        the returned list are then None.  `last`: this is the last stage VJP of a reversed step (lambda is rewritten next)."""
        if slot is not None and self._sg is not None and which == "EX" and alpha is not None:
            return self._sg.vjp(self, slot, t, y_flat, w_flat, tape, alpha, last)
        lin = self._lin if (which == "EX" and self._lin is not None) else None
        all_params = self._paramsI if which == "IM" else self._paramsE
        # (a tape that belongs to a captured evaluation is differentiated again at every replay of its backward unit)
        keep = True if (self._unit_capture and tape is not None) else None
        tt = None
        if tape is not None:
            y, out, wrt = tape[:3]
            tt = tape[3] if len(tape) > 3 else None
        else:
            self.nfe_backward += 1
        with torch.enable_grad() if tape is None else contextlib.nullcontext():
            if tape is None:
                y = self._shaped(y_flat).detach().requires_grad_(True)
                if self._tgrad and which == "EX":
                    tt = self._t_arg(t, True)
                out, wrt = self._func_with_grad(t if tt is None else tt, y, which)
            cot = self._shaped(w_flat).view(out.shape)
            # dL/dt: t is one more input of this backward pass; <w, K> is taken before anything rewrites w
            tgx = (tt,) if (tt is not None and self._tg is not None and which == "EX") else ()
            gt = None
            if tgx:
                self._tg_dot(slot, w_flat, out, alpha)
            hooked = lin is not None and len(wrt) != len(all_params)      # this evaluation left the Linear layers to the hooks
            if hooked and not lin.disabled and alpha is not None:
                capturing = self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
                if not lin.checked and not capturing:
                    ok, worst = lin.self_check(self, out, y, all_params, cot)
                    if not ok:
                        lin.disabled = True
                        lin.why = "its result differed from autograd's at the self-check (relative %.1e)" % worst
                        lin.remove_hooks_only()
                        warnings.warn("pnode_amd: the engine-side accumulation of the nn.Linear layers' parameter sensitivities is "
                                      "switched off for this solver: its result differs from autograd's (relative %.1e) -- a "
                                      "weight or bias of such a layer is also used somewhere else in func.  Results are autograd's; "
                                      "-pn_linear_param_grads 0 silences this." % worst, RuntimeWarning)
                if not lin.disabled:
                    # The hooks add to mu during this backward pass (or queue bias sums behind what is queued already); parameter
                    # cotangents autograd formed for EARLIER stages -- evaluations the structural check left to it -- may still
                    # wait in the batched queue: add them first, so that mu sees every stage's contribution in the order of
                    # the stages whatever -pn_param_accum says (the same bits in every mode, also for a func that mixes the two
                    # kinds of evaluation in one solve)
                    if self._pend_g and self._pend_mixed:
                        self._flush_param_accum()
                    lin.alpha, lin.target = float(alpha), self.adj_p_tensor
                    lin.cot_storage = w_flat.untyped_storage().data_ptr()
                    try:
                        grads = torch.autograd.grad(out, (y,) + wrt + tgx, cot, allow_unused=True, retain_graph=keep)
                    finally:
                        lin.alpha = None
                    if tgx:
                        gt, grads = grads[-1], grads[:-1]
                    grads = (grads[0],) + tuple(lin.expand(grads[1:], len(all_params)))
                    hooked = None
            if hooked:
                # evaluated with the hooks on, differentiated without them (the self-check failed, or a caller that adds the
                # parameter cotangents itself): autograd differentiates with respect to every parameter
                if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    raise PnError("pnode_amd: a stage evaluation recorded for the engine-side Linear accumulation cannot be "
                                  "differentiated by autograd alone inside a hipGraph capture")
                lin.muted = True
                try:
                    grads = torch.autograd.grad(out, (y,) + tuple(all_params) + tgx, cot, allow_unused=True, retain_graph=keep)
                finally:
                    lin.muted = False
                if tgx:
                    gt, grads = grads[-1], grads[:-1]
            elif hooked is False:
                grads = torch.autograd.grad(out, (y,) + wrt + tgx, cot, allow_unused=True, retain_graph=keep)
                if tgx:
                    gt, grads = grads[-1], grads[:-1]
                if lin is not None:
                    self._pend_mixed = True            # what the caller queues now holds cotangents of parameters the hooks also serve
                    if self._pend_bias:
                        self._flush_bias_accum()       # (the mirror case: bias sums queued by the hooks of earlier stages go first)
            if lin is not None:
                # the stage's queued (cotangent, input) pairs: one grouped launch of the fused kernel, beside the next stage; the
                # launches of earlier stages are waited for (every stage VJP, also one autograd did alone: the buffers turn)
                lin.flush(self, lam=self.adj_u_flat if last else None)
            if tgx:
                self._tg_tbar(slot, gt, alpha)
        return self._vjp_results(grads[0], grads[1:], w_flat, deferred=self._accum_mode != "stage")

    def _vjp_results(self, gy, grads, cotangent, deferred=True):
        """What autograd returned for a stage VJP as the sweeps take it: J^T w flat, the parameter cotangents as a list, all in the
        state's dtype and contiguous (a None stays None).  Deferred accumulation (-pn_param_accum batch|step, the per-sample sweep)
        reads the parameter cotangents launches later, after the buffer of `cotangent` (w_a, or lambda itself for a folded stage)
        has been rewritten in place.  Autograd hands the cotangent, or ANY view of it, straight through for f = ... + p,
        cat([z[:2] + b1, ...]), stack((.. + p0, ..)): every gradient that shares the cotangent's storage is copied, whatever its size.
        `deferred` False (-pn_param_accum stage): they are added before anything rewrites the buffer, nothing is copied."""
        dt = self.tensor_dtype
        if gy is not None:
            if gy.dtype != dt:
                gy = gy.to(dt)
            gy = gy.contiguous().reshape(-1)
        wst = cotangent.untyped_storage().data_ptr() if deferred else None
        gp = []
        for g in grads:
            if g is not None:
                if g.dtype != dt or not g.is_contiguous():
                    g = g.to(dt).contiguous()
                if wst is not None and g.untyped_storage().data_ptr() == wst:
                    g = g.clone()
            gp.append(g)
        return gy, gp

    def _adjoint_steps(self, nsteps, forcing, dense_w=None):
        """TSAdjointSolve over `nsteps` steps, newest first (TSAdjointStep_RK per step), then
        add `forcing` (dL/dy at the span point reached; pa.py:938) fused into the last update.

        Per step [t_n, t_n+H] with stage values Y_i, incoming lambda and mu:
            for i = s-1 .. 0:   w_i = H*(b_i*lambda + sum_{j>i} a_ji*dlam_j)
                                (dlam_i, dmu_i) = VJP of f at Y_i with cotangent w_i
            mu     <- mu + sum_i dmu_i      (stages added in the order s-1..0: one multi-tensor launch per
                                             stage, or per time step with -pn_param_accum step; same rounding)
            lambda <- lambda + sum_i dlam_i
        (the scale PETSc applies after MatMultTranspose is applied to the cotangent instead).
        A stage whose cotangent is a pure multiple of lambda -- the last non-trivial stage of
        every tableau -- is differentiated with lambda itself and the scalar is folded into
        the coefficients of everything that consumes its result: no kernel, no extra vector.

        `dense_w` (-pn_output_times interpolate, one step): per stage the cotangent D_i its interpolated outputs send it, or
        None; added to w_i as the last term (a stage with a D_i is always formed, pn_rk_adjoint_step_dense)."""
        if self._theta is not None:
            return self._theta.adjoint_steps(nsteps, forcing)
        if nsteps == 0 and forcing is not None:
            self._ops.adj_accum(self.adj_u_flat, self.adj_u_flat, [], [], forcing)
        # two cotangent buffers in turn while the weight-sensitivity products of a stage run beside the next stage on a second
        # stream (pnode_amd/_lineargrad.py): the product of stage i reads stage i's cotangent while stage i-1's is written
        two_w = self._lin is not None and self._lin.side_on
        reversed_step = self._adjoint_step_native if self._native else self._adjoint_step_python
        for r in range(nsteps):
            step = self._rev_next
            tn, H = self._step_info(step)
            if self._tg is not None:
                self._tg["cur"] = step
            if self._lin is not None and self._tmode != _lib.PN_TRAJ_ALL:
                self._lin.join()             # a product still running may read stage values the recomputation below rewrites
            Y = self._stages_of(step)
            tapes = self._tapes.pop(step, None) if self._tapes else None
            if tapes is None and self._rtapes is not None:
                tapes = self._rtapes             # recorded while the stage values were recomputed (_stages_of)
            self._rtapes = None
            dlam = [None] * self._s          # raw VJP results
            reversed_step(step, tn, H, Y, tapes, dlam, forcing if r == nsteps - 1 else None, dense_w, two_w)
            self._traj.rev_done(step)
            self._rev_next = step - 1

    def _flush_after_step(self):
        """What a reversed step's stage VJPs queued for mu, once they have all run: added now (oldest first, one launch) with
        -pn_param_accum step, with per-evaluation graphs (the cotangents sit in static outputs) and when the queue is full."""
        if self._pend_g and (self._accum_mode == "step" or self._sg is not None or len(self._pend_g) + self._s_eff > self._accum_cap):
            self._flush_param_accum()
        elif self._pend_bias and self._accum_mode == "step":
            self._flush_bias_accum()

    def _adjoint_step_native(self, step, tn, H, Y, tapes, dlam, forcing, dense_w, two_w):
        """One reversed step by the C++ loop (pn_rk_adjoint_step; with `dense_w` pn_rk_adjoint_step_dense), which calls back for
        the stage VJPs only."""
        ops, lam = self._ops, self.adj_u_flat
        if getattr(self, "_vjp_cb_c", None) is None:
            self._make_callbacks()
        self._rcbs = (Y, tapes, dlam, self._first_stage_time(step))
        args = (ops.stream(), ops.code, self.n, self._ts, ops.vec_ops, tn, H, lam.data_ptr(), self._buf("w_a").data_ptr(),
                self._buf("w_b").data_ptr() if two_w else None, self._vjp_cb_c, None)
        fo = None if forcing is None else forcing.data_ptr()
        if dense_w is not None:
            dw = (ctypes.c_void_p * _lib.PN_MAX_STAGES)(*[None if d is None else d.data_ptr() for d in dense_w])
            rc = self._lib.pn_rk_adjoint_step_dense(*(args + (dw, fo)))
        else:
            rc = self._lib.pn_rk_adjoint_step(*(args + (fo,)))
        self._rcbs = None
        if rc:
            self._raise_from_loop(rc)
        self._flush_after_step()

    def _adjoint_step_python(self, step, tn, H, Y, tapes, dlam, forcing, dense_w, two_w):
        """One reversed step with the stage loop in Python, one call per launch: the same launches, coefficients and bits."""
        ops, s_eff, A, b = self._ops, self._s_eff, self._A, self._b
        lam = self.adj_u_flat
        scale = [1.0] * self._s          # true dlam_i = scale[i] * dlam[i]
        nw = 0
        for i in range(s_eff - 1, -1, -1):
            js = [j for j in range(i + 1, s_eff) if A[j][i] != 0.0 and dlam[j] is not None]
            di = dense_w[i] if dense_w is not None else None
            if b[i] == 0.0 and not js and di is None:
                continue                   # structurally zero cotangent
            if not js and di is None:
                w, scale[i] = lam, H * b[i]
            else:
                w = self._buf("w_b" if (two_w and nw % 2) else "w_a")
                nw += 1
                ops.adj_theta(w, lam if b[i] != 0.0 else None, H * b[i],
                              [dlam[j] for j in js] + ([di] if di is not None else []),
                              [H * A[j][i] * scale[j] for j in js] + ([1.0] if di is not None else []))
            # (stage 0 of a first-same-as-last tableau was evaluated at the previous step's last stage time, which is
            # t_n only to the last bit: the VJP differentiates f THERE, with and without a tape -- the exact discrete
            # adjoint, the same bits in every checkpoint mode for a time-dependent f; PETSc passes t_n)
            t0 = self._first_stage_time(step) if i == 0 else None
            gy, gp = self._vjp(tn + self._c[i] * H if t0 is None else t0, Y[i], w, tapes[i] if tapes else None, alpha=scale[i], last=(i == 0), slot=i)
            if tapes:
                tapes[i] = None            # release the stage's activations as soon as they are used
            if gy is not None and gy.data_ptr() == w.data_ptr():
                gy = gy.clone()            # f returned its cotangent unchanged (identity-like f)
            dlam[i] = gy
            self._take_param_grads(scale[i], gp, deferred=self._accum_mode != "stage")
        self._flush_after_step()           # (before lambda's update: the launches keep their order)
        idx = [i for i in range(s_eff) if dlam[i] is not None]
        ops.adj_accum(lam, lam, [dlam[i] for i in idx], [scale[i] for i in idx], forcing)

    def _take_param_grads(self, scale, gp, deferred=True):
        """mu += scale * gp, the parameter cotangents of one stage VJP: queued for the batched launch of _flush_param_accum, or
        (-pn_param_accum stage) added at once."""
        if self.np > 0 and any(g is not None for g in gp):
            if deferred:
                self._pend_a.append(scale)
                self._pend_g.append(gp)
            else:
                self._ops.param_accum(self.adj_p_tensor, scale, gp, self._poff, self._plen)

    def _add_param_grads(self, alpha, gp, first=0, stable=True, cotangent=None):
        """mu[parameters first .. first+len(gp)) += alpha * gp for the implicit / IMEX steppers: one launch per call with
        -pn_param_accum stage, else queued for the batched launch of _flush_param_accum (same order, same rounding).
        `stable` False: the gradients sit in buffers that are rewritten before a deferred launch would read them (the
        outputs of a replayed graph): what is queued is added first, then these, at once.  `cotangent`: the buffer the
        gradients were computed FROM when they did not come through _vjp -- a gradient that is a view of it is copied."""
        if not any(g is not None for g in gp):
            return
        n_all = len(self._poff)
        full = first == 0 and len(gp) == n_all
        if self._accum_mode == "stage" or not stable:
            self._flush_param_accum()
            if full:
                off, ln = self._poff, self._plen
            elif first == 0:
                off, ln = self._poffI, self._plenI
            else:
                off, ln = self._poffE, self._plenE
            self._ops.param_accum(self.adj_p_tensor, alpha, list(gp), off, ln)
            return
        if cotangent is not None:
            gp = self._vjp_results(None, gp, cotangent)[1]
        self._pend_a.append(alpha)
        self._pend_g.append(list(gp) if full else [None] * first + list(gp) + [None] * (n_all - first - len(gp)))
        if len(self._pend_g) >= self._accum_cap:
            self._flush_param_accum()

    def _colsum_accum(self, g2, mu_slice, alpha):
        """mu_slice += alpha * column sums of g2 (rows x cols): the sensitivity of a bias.  Queued like the parameter
        cotangents of autograd (-pn_param_accum batch|step: the cotangent tensors stay alive, at most 1 GiB of them, and up to
        32 are summed by ONE pn_colsum_accum_multi pass; stage: at once) -- same bits whatever the grouping."""
        g2 = g2.contiguous()
        self._pend_bias.append((g2, mu_slice, float(alpha)))
        self._pend_bias_bytes += g2.numel() * g2.element_size()
        if self._accum_mode == "stage" or len(self._pend_bias) >= 32 or self._pend_bias_bytes >= (1 << 30):
            self._flush_bias_accum()

    def _flush_bias_accum(self):
        if self._pend_bias:
            fn = getattr(self._ops, "colsum_accum_multi", None)
            if fn is not None and self._pend_bias[0][0].device.type == "cuda":
                fn(self._pend_bias)
            else:                                        # the CPU test stand-in: same order, double sums
                for g2, mu_slice, alpha in self._pend_bias:
                    mu_slice.add_(g2.double().sum(0).to(mu_slice.dtype), alpha=alpha)
            self._pend_bias = []
            self._pend_bias_bytes = 0

    @property
    def linear_param_grads(self):
        """How the parameter sensitivities of func's nn.Linear layers are formed: "engine (N parameters)" or "autograd (why)"."""
        lin = self._lin
        if lin is None:
            return "autograd (no eligible nn.Linear layer, a theta stepper, or -pn_linear_param_grads 0)"
        if lin.disabled:
            return "autograd (%s)" % lin.why
        note = "; fused dW + db MFMA kernel on %d layers" % len(lin.partials) if lin.partials else ""
        if lin.n_autograd:
            # the structural check (LinearParamGrads.end): evaluations in which a handled parameter was also used outside its layer
            note += "; %d of %d recorded evaluations of func left to autograd (a handled weight or bias is also used outside its layer there, " \
                    "or a layer runs in another precision than its parameters -- autocast)" % (lin.n_autograd, lin.n_autograd + lin.n_clean)
        return "engine (%d of %d parameter tensors%s)" % (len(lin.handled), len(self._paramsE), note)

    def _setup_linear_grads(self):
        """(Re)install the engine-side accumulation of func's nn.Linear layers (pnode_amd/_lineargrad.py): explicit RK path
        only; -pn_linear_param_grads auto|gemm|0 (not a PETSc option)."""
        opt = str(options.get_all().get("pn_linear_param_grads", "auto"))
        gemm = opt == "gemm"             # the library GEMM + pn_colsum_accum_multi for every layer (no fused MFMA kernel)
        on = opt in ("auto", "gemm") or options.truthy(opt, False)
        # explicit RK (func), and ARKIMEX's explicitly treated func2: the only grad-enabled evaluations of that function are the
        # solver's own taped stage evaluations and stage VJPs.  Not the theta methods: their Newton-Krylov solves differentiate
        # func in ways of their own (double VJPs, captured linearisations)
        side = str(options.get_all().get("pn_linear_side_stream", "0"))
        # -pn_linear_side_stream 1 | same-priority (default 0): the products on a second stream beside the next stage's backward
        # pass -- the explicit RK sweep only (its cotangent buffers are doubled for it); ARKIMEX's stage vectors are rewritten on a
        # schedule of their own.  Measured at BASELINE's target configuration (profiles/r06_side_stream.txt): +1.5 % time-steps/s,
        # the same bits; the dX GEMMs of the next stage take 36 us beside the product against 19.4 alone -- the two share the
        # matrix pipes -- and every kernel's own duration stops being a statement about that kernel, so it is not the default.
        side_on = (side == "same-priority" or options.truthy(side, False)) and self._stepper_kind is None and self.device.type == "cuda"
        # -pn_linear_wgrad_exact 1: fp32 states on the fp32 matrix instruction (a k-ordered fmaf chain) instead of the default --
        # operands split exactly into three bf16 terms, six bf16 MFMA products per fp32 product, fp32 accumulation (csrc/pn_linear.hip)
        exact = options.truthy(options.get_all().get("pn_linear_wgrad_exact", 0), False)
        # -pn_linear_wgrad_tile64 1: the split-bf16 form always on 64 x 64 workgroup tiles (by default a launch that fills whole rounds
        # of the chip takes 128 x 128 ones; the same bits) -- for comparisons
        tile64 = options.truthy(options.get_all().get("pn_linear_wgrad_tile64", 0), False) or side_on
        # (the second stream implies the small tiles: a 128 x 128 workgroup holds a CU's whole LDS, nothing runs beside it -- measured
        # 869 against 958 time-steps/s; with 64 x 64 tiles the second stream is worth +1.5 %, profiles/r06_side_stream.txt)
        if hasattr(self._ops, "wgrad_flags"):
            self._ops.wgrad_flags = (_lib.PN_WGRAD_EXACT_FP32 if exact else 0) | (_lib.PN_WGRAD_TILE_64 if tile64 else 0)
        self._setup_linear_fwd()
        sig = (id(self.funcEX), on, self._stepper_kind in (None, "imex"), tuple(id(p) for p in self._paramsE), gemm, side_on, exact, tile64)
        if sig == self._lin_sig:
            return
        self._lin_sig = sig
        if self._lin is not None:
            self._lin.remove()
            self._lin = None
        if on and sig[2] and self._paramsE:
            from ._lineargrad import LinearParamGrads
            lin = LinearParamGrads(self)
            lin.fused = not gemm
            lin.side_on = side_on
            lin.side_priority = side != "same-priority"
            if lin.install(self.funcEX, self._paramsE, self._poffE if self._stepper_kind == "imex" else self._poff):
                self._lin = lin

    def _setup_linear_fwd(self):
        """(Re)install the fused forward of func's Linear -> Tanh pairs (pnode_amd/_linearfwd.py): explicit RK path and ARKIMEX's
        func2, as the engine-side sensitivities; -pn_linear_fwd auto|0|1 (not a PETSc option).  -pn_linear_bwd auto|0|1: the backward
        of the same pairs as one launch each (pn_linear_bwd); it lives in the pair's Function, so it has no effect without the forward.
        -pn_linear_bare 0|1 (default 0): func's bare nn.Linear layers through pn_linear_fwd with the identity and pn_linear_dx.
        -pn_linear_relu 0|1 (default 0; anything else is refused): func's Linear -> ReLU pairs as the Tanh ones.
        -pn_linear_sigmoid 0|1 (default 0; anything else is refused): func's Linear -> Sigmoid pairs as the Tanh ones.
        -pn_linear_gelu 0|1 (default 0; anything else is refused): func's Linear -> GELU pairs, which save their pre-activation.
        -pn_linear_softplus 0|1, -pn_linear_elu 0|1 (default 0; anything else is refused): func's Linear -> Softplus (beta 1, threshold
        20) and Linear -> ELU (alpha 1) pairs as the Sigmoid ones."""
        mode = str(options.get_all().get("pn_linear_fwd", "auto"))
        mode = "auto" if mode == "auto" else ("1" if options.truthy(mode, False) else "0")
        bwd = str(options.get_all().get("pn_linear_bwd", "auto"))
        bwd = "auto" if bwd == "auto" else ("1" if options.truthy(bwd, False) else "0")
        # -pn_linear_form auto|plain: `plain` keeps the plain K loop of both kernels on aligned shapes too (PN_LINEAR_FORM_PLAIN; the
        # same bits as the pipelined loop they take by themselves) -- for comparisons inside one tree
        bare = "1" if options.truthy(options.get_all().get("pn_linear_bare", "0"), False) else "0"
        from ._linearfwd import PAIRS, LinearFwd
        # -pn_linear_<key> 0|1 (default 0) of every kind of pair beside the tanh pairs: through pn_linear_fwd (pn_linear_fwd_pre) with the
        # kind's PN_ACT_* code and pn_linear_bwd_act
        acts = []
        for kind in PAIRS:
            if not kind.always:
                acts.append(str(options.get_all().get(kind.option[1:], "0")))
                if acts[-1] not in ("0", "1"):
                    raise PnError("%s must be 0 or 1 (got '%s')" % (kind.option, acts[-1]))
        form = options.linear_form()
        if hasattr(self._ops, "linear_flags"):
            self._ops.linear_flags = _lib.PN_LINEAR_FORM_PLAIN if form == "plain" else 0
        on = mode != "0" and self._stepper_kind in (None, "imex") and self.device.type == LinearFwd.device_type \
            and self.tensor_dtype == torch.float32 and hasattr(self._ops, "linear_fwd")
        sig = (id(self.funcEX), mode, on, tuple(id(p) for p in self._paramsE), bwd, form, bare) + tuple(acts)
        if sig == self._fwd_sig:
            return
        self._fwd_sig = sig
        self._fwd = None
        if on and self._paramsE:
            fwd = LinearFwd(self)
            if fwd.install(self.funcEX, self._paramsE, mode, bwd, bare, *acts):
                self._fwd = fwd

    @property
    def linear_fwd(self):
        """How func's Linear -> Tanh pairs run in the solver's evaluations: "fused (N pairs)" or "stock modules (why)"."""
        fwd = self._fwd
        if fwd is None or not fwd.plans:
            return "stock modules (no eligible pair, not an fp32 state on a HIP device, a theta stepper, or -pn_linear_fwd 0)"
        if fwd.disabled:
            return "stock modules (%s)" % fwd.why
        return "fused (%d pairs, %d calls so far)" % (sum(len(p) for _, p in fwd.plans), fwd.n_fused)

    @property
    def linear_bwd(self):
        """How the backward of those pairs runs: "fused (N calls so far)" or "torch operations (why)"."""
        fwd = self._fwd
        if fwd is None or fwd.disabled or not fwd.plans:
            return "torch operations (the pairs run the stock modules: see linear_fwd)"
        return fwd.bwd_status

    @property
    def linear_bare(self):
        """How func's bare nn.Linear layers run in the solver's evaluations: "off (-pn_linear_bare 0)", "fused (N layers; F forward,
        R backward calls so far)" or "stock modules (why)"."""
        fwd = self._fwd
        if fwd is None:
            bare = options.truthy(options.get_all().get("pn_linear_bare", "0"), False)
            return "stock modules (no eligible layer, not an fp32 state on a HIP device, a theta stepper, or -pn_linear_fwd 0)" if bare \
                else "off (-pn_linear_bare 0)"
        return fwd.bare_status

    @property
    def linear_relu(self):
        """How func's nn.Linear -> nn.ReLU pairs run in the solver's evaluations: "off (-pn_linear_relu 0)", "fused (N pairs; F forward,
        R backward calls so far)" or "stock modules (why)"."""
        return self._pair_status("relu")

    @property
    def linear_sigmoid(self):
        """How func's nn.Linear -> nn.Sigmoid pairs run in the solver's evaluations: "off (-pn_linear_sigmoid 0)", "fused (N pairs; F
        forward, R backward calls so far)" or "stock modules (why)"."""
        return self._pair_status("sigmoid")

    @property
    def linear_gelu(self):
        """How func's nn.Linear -> nn.GELU pairs run in the solver's evaluations: "off (-pn_linear_gelu 0)", "fused (N pairs; F forward, R
        backward calls so far)" or "stock modules (why)"."""
        return self._pair_status("gelu")

    def _pair_status(self, name):
        fwd = self._fwd
        if fwd is None:
            return "stock modules (no eligible pair, not an fp32 state on a HIP device, a theta stepper, or -pn_linear_fwd 0)" \
                if str(options.get_all().get("pn_linear_" + name, "0")) == "1" else "off (-pn_linear_%s 0)" % name
        return fwd.records[name].status

    @property
    def linear_softplus(self):
        """How func's nn.Linear -> nn.Softplus pairs (beta 1, threshold 20) run in the solver's evaluations: "off (-pn_linear_softplus
        0)", "fused (N pairs; F forward, R backward calls so far)" or "stock modules (why)"."""
        return self._pair_status("softplus")

    @property
    def linear_elu(self):
        """How func's nn.Linear -> nn.ELU pairs (alpha 1) run in the solver's evaluations: "off (-pn_linear_elu 0)", "fused (N pairs; F
        forward, R backward calls so far)" or "stock modules (why)"."""
        return self._pair_status("elu")

    def _flush_param_accum(self):
        self._flush_bias_accum()
        self._pend_mixed = False
        if self._pend_g:
            self._ops.param_accum_multi(self.adj_p_tensor, self._pend_a, self._pend_g, self._poff, self._plen)
            del self._pend_a[:], self._pend_g[:]

    def _begin_adjoint(self, seed):
        if self._traj is None:
            raise RuntimeError("adjoint requested but no trajectory was saved "
                               "(setupTS(enable_adjoint=True) and a differentiable input are required)")
        if self.adj_u_tensor is None:
            self.adj_u_tensor = self._ops.empty(self._npad)
        self.adj_u_flat = self.adj_u_tensor
        self._ops.copy(self.adj_u_flat, seed)
        self._begin_param_adjoint()
        self._traj.begin_reverse()
        self._rev_next = self._nsteps - 1
        if self._lin is not None:
            self._lin.reset()              # (partial sums a sweep that raised may have left behind)

    def _begin_param_adjoint(self):
        """mu = 0 and nothing queued for it: the start of every reverse sweep, the per-sample one included."""
        if self.adj_p_tensor is None or self.adj_p_tensor.numel() != self.np:
            self.adj_p_tensor = self._ops.empty(max(self.np, 1))[: self.np]
        self.adj_p_tensor.zero_()
        self._pend_a, self._pend_g = [], []
        self._pend_mixed = False             # the queue holds autograd's cotangents of parameters the Linear hooks also serve
        self._pend_bias, self._pend_bias_bytes = [], 0
        # pending stage results are kept alive until they are added: bound them to 1 GiB
        esize = 4 if self.tensor_dtype == torch.float32 else 8
        self._accum_cap = max(1, min(self._accum_sources, (1 << 30) // max(self.np * esize, 1)))

    def _reverse_sweep(self, g, T):
        """The body of OdeintAdjointMethod.backward (pa.py:924-944) on the (T, n) cotangent."""
        return self._traced("pnode_amd.reverse_sweep", self._reverse_sweep_impl, g, T)

    def _reverse_sweep_impl(self, g, T):
        self._tg = None
        if self._sample:
            return self._rows_reverse(g, T)
        if self._tgrad:
            self._tg_begin(T)
        if self._dense_active:
            return self._reverse_sweep_dense(g, T)
        self._begin_adjoint(g[T - 1])
        if T == 1:
            self._adjoint_steps(self._nsteps, None)
        for i in range(T - 1, 0, -1):
            self._adjoint_steps(self.cur_sol_steps[i], g[i - 1])
        self._flush_param_accum()
        self._finish_linear_accum()

    def _dense_rows(self, T):
        """Per step n: (lo, hi, coefficient rows) -- the output times t_n <= t[o] < t_{n+1}, o < T-1, and per output h*beta_j(theta)
        for every stage (None: the output IS the state at t_n).  From the step log and the output times only, as the forward sweep
        classified them."""
        times = self.sol_times.tolist()
        N = self._nsteps
        log = [self._step_info(k) for k in range(N)]
        rows, o = [], 0
        for k in range(N):
            tn, h = log[k]
            tend = log[k + 1][0] if k + 1 < N else times[T - 1]
            lo = o
            while o < T - 1 and times[o] < tend:
                o += 1
            rows.append((lo, o, [None if times[q] == tn else self._dense_coefs(times[q], tn, h) for q in range(lo, o)]))
        return log, rows

    def _reverse_sweep_dense(self, g, T):
        """The reverse sweep of a solve with interpolated outputs: per reversed step n, its outputs' cotangents
        g_o give D_j = sum_o h beta_j(theta_o) g_o (stage j's extra cotangent) and G = sum_o g_o (added to lambda_n in the closing
        update, with the g of an output AT t_n).  First same as last: K_{s-1} of step n is K_0 of step n+1, so step n's column s-1
        goes into D_0 of step n+1; for the last step, one extra VJP at (y_N, t_{N-1} + c_{s-1} h) before the sweep."""
        ops, s = self._ops, self._s
        self._begin_adjoint(g[T - 1])
        log, rows = self._dense_rows(T)
        N = len(rows)
        fs = s - 1 if self._fsal else None
        cols = [j for j in self._dense_cols if j != fs]

        def interior(k):
            return any(c is not None for c in rows[k][2])

        def fsal_part(k):            # rows of step k and their column s-1
            lo, hi, cf = rows[k]
            return g[lo:hi], [[0.0 if c is None else c[fs]] for c in cf]

        if fs is not None and N > 0 and interior(N - 1):
            d = self._buf("dense_fsal")
            gk, cf = fsal_part(N - 1)
            ops.dense_adjoint([d], None, gk, cf)
            tl, hl = log[N - 1]
            if self._tg is not None:
                self._tg.update(cur=N - 1, yN=True)
            gy, gp = self._vjp(tl + self._c[fs] * hl, self._buf("dense_yN"), d, None, alpha=1.0)
            if self._tg is not None:
                self._tg["yN"] = False
            if gy is not None:
                ops.adj_accum(self.adj_u_flat, self.adj_u_flat, [gy], [1.0], None)
            self._take_param_grads(1.0, gp, deferred=self._accum_mode != "stage")
        for k in range(N - 1, -1, -1):
            lo, hi, cf = rows[k]
            dw = [None] * _lib.PN_MAX_STAGES
            G = None
            if hi > lo:
                G = self._buf("dense_G")
                if interior(k):
                    Ds = [self._buf("dense_d%d" % j) for j in cols]
                    ops.dense_adjoint(Ds, G, g[lo:hi], [[0.0 if c is None else c[j] for j in cols] for c in cf])
                    for j, d in zip(cols, Ds):
                        dw[j] = d
                else:
                    ops.dense_adjoint([], G, g[lo:hi], [[] for _ in cf])
            if fs is not None and k > 0 and interior(k - 1):
                d0 = self._buf("dense_d0")
                gk, cfk = fsal_part(k - 1)
                ops.dense_adjoint([d0], None, gk, cfk, accumulate=dw[0] is not None)
                dw[0] = d0
                if self._tg is not None and k == N - 1:
                    # the part of stage 0's cotangent that step k-1's outputs send to its last stage scales with H_{k-1}, not
                    # with H_k: <., K> of it is taken off the last step's dL/dH
                    fp = self._tg["fprev"] = self._buf("dense_tg_fprev")
                    ops.dense_adjoint([fp], None, gk, cfk)
            self._adjoint_steps(1, G, dense_w=dw if any(d is not None for d in dw) else None)
            if self._tg is not None:
                self._tg["fprev"] = None
                self._tg_dense_step(k, g, log, rows)
        self._flush_param_accum()
        self._finish_linear_accum()

    # ------------------------------------------------------------------ dL/dt
    def _tgrad_supported(self):
        """Whether odeint_adjoint's backward returns dL/dt: explicit RK, not under -pn_reference_defaults (the reference's
        None, pa.py:947).  The theta / IMEX steppers return None too and say so once per solver."""
        if self._ref_defaults:
            return False
        if self._theta is not None:
            if not self._tg_warned:
                self._tg_warned = True
                warnings.warn("pnode_amd: the gradient with respect to the output times t is returned for the explicit RK "
                              "steppers only; this solver's %s stepper returns None for it" % (self._stepper_kind or "implicit"),
                              RuntimeWarning, stacklevel=4)
            return False
        return True

    def _t_arg(self, t, grad):
        """The time argument of func in a solve that differentiates with respect to t: a 0-dim float64 tensor on the
        state's device (the form the per-evaluation graphs hand over), a leaf that requires grad where autograd follows."""
        tt = torch.full((), float(t), dtype=torch.float64, device=self.device)
        return tt.requires_grad_(True) if grad else tt

    def _tg_begin(self, T):
        """Accumulators of one reverse sweep: per output interval i, P[i] = dL/dH of its last step and Q[i] = sum of dL/dtau
        over its steps; per interpolated output o, E[o] = dL/dt_o.  One fp64 device vector, read once by _tg_finish."""
        N = self._nsteps
        dense = self._dense_active
        counts = [N] if (dense or T == 1) else list(self.cur_sol_steps[1:T])
        iv, last, k = [0] * N, set(), 0
        for i, c in enumerate(counts, 1):
            for _ in range(c):
                iv[k] = i
                k += 1
            if c:
                last.add(k - 1)
        ni = len(counts)
        acc = torch.zeros(2 * (ni + 1) + T, dtype=torch.float64, device=self.device)
        self._tg = dict(acc=acc, iv=iv, last=last, ni=ni, T=T, dense=dense, cur=0, yN=False, fprev=None, K={}, theta_last=[])

    def _tg_owner(self, slot):
        """(step whose tau and H the time argument of this stage evaluation depends on, its c)."""
        tg = self._tg
        k = tg["cur"]
        if tg["yN"]:
            return k, self._c[self._s - 1]
        if self._fsal and slot == 0 and k > 0:
            return k - 1, self._c[self._s - 1]       # first same as last: evaluated by the previous step
        return k, self._c[slot]

    def _tg_dot(self, slot, w_flat, out, alpha):
        """<w, K>/H of a stage of the last step of an output interval goes to that interval's dL/dH (pn_tgrad_dots)."""
        tg = self._tg
        k = tg["cur"]
        K = out.detach().reshape(-1)
        if not K.is_contiguous():
            K = K.contiguous()
        if tg["dense"]:
            owner, _ = self._tg_owner(slot)
            j = self._s - 1 if owner != k or tg["yN"] else slot
            tg["K"][(owner, j)] = K
            if owner != k:
                tg["K"][(k, 0)] = K
        if k not in tg["last"]:
            return
        H = self._step_info(k)[1]
        a = 1.0 if alpha is None else float(alpha)
        xs, ys, cs = [w_flat], [K], [a / H]
        if tg["fprev"] is not None and not tg["yN"] and slot == 0:
            xs.append(tg["fprev"])
            ys.append(K)
            cs.append(-1.0 / H)
        i = tg["iv"][k]
        self._ops.tgrad_dots(tg["acc"][i:i + 1], xs, ys, cs)

    def _tg_tbar(self, slot, gt, alpha):
        """T = <w, df/dt>: dL/dtau of the step that evaluated the stage, and c times it to dL/dH when that step ends an interval."""
        if gt is None:
            return                                     # func's output does not reach t (autonomous func)
        tg = self._tg
        owner, c = self._tg_owner(slot)
        a = 1.0 if alpha is None else float(alpha)
        i = tg["iv"][owner]
        acc = tg["acc"]
        acc[tg["ni"] + 1 + i].add_(gt.to(torch.float64), alpha=a)
        if owner in tg["last"] and c != 0.0:
            acc[i].add_(gt.to(torch.float64), alpha=a * c)

    def _tg_dense_step(self, k, g, log, rows):
        """e_o = <g_o, sum_j beta'_j(theta_o) K_j> for the interpolated outputs of step k, once its K_j are known (pn_rk_dense_tgrad)."""
        tg = self._tg
        lo, hi, _ = rows[k]
        Kk = {j: v for (st, j), v in tg["K"].items() if st == k}
        for key in [key for key in tg["K"] if key[0] == k]:
            del tg["K"][key]
        if hi == lo:
            return
        times = self.sol_times.tolist()
        tn, h = log[k]
        ths = [(times[o] - tn) / h for o in range(lo, hi)]
        P = self._dense_P
        dcoef = [[sum((p + 1) * P[j][p] * th ** p for p in range(len(P[j]))) for j in range(self._s)] for th in ths]
        cols = [j for j in range(self._s) if any(r[j] != 0.0 for r in dcoef)]
        missing = [j for j in cols if j not in Kk]
        if missing:
            raise PnError("pnode_amd: dL/dt of interpolated outputs: stage derivative(s) %s of step %d were not evaluated" % (missing, k))
        base = 2 * (tg["ni"] + 1)
        self._ops.dense_tgrad(tg["acc"][base + lo:base + hi], g[lo:hi], [Kk[j] for j in cols],
                              [[r[j] for j in cols] for r in dcoef])
        if k in tg["last"]:
            tg["theta_last"] = list(zip(range(lo, hi), ths))

    def _tg_finish(self, t):
        """dL/dt from the accumulators (one read): dL/dt_0 = Q_1 - P_1, dL/dt_i = P_i - P_{i+1} + Q_{i+1}, dL/dt_N = P_N; an
        interpolated output o adds e_o to its own entry and takes it from tau of its step (and theta_o e_o from the last H)."""
        tg, self._tg = self._tg, None
        a = tg["acc"].cpu().tolist()
        ni, T = tg["ni"], tg["T"]
        P = a[:ni + 1]
        Q = a[ni + 1:2 * (ni + 1)]
        E = a[2 * (ni + 1):]
        out = [0.0] * T
        if tg["dense"]:
            for o in range(1, T - 1):
                out[o] = E[o]
                Q[1] -= E[o]
            for o, th in tg["theta_last"]:
                P[1] -= th * E[o]
            out[0], out[T - 1] = Q[1] - P[1], P[1]
        elif T == 1:
            out[0] = P[1]
        else:
            out[0] = Q[1] - P[1]
            for i in range(1, T - 1):
                out[i] = P[i] - P[i + 1] + Q[i + 1]
            out[T - 1] = P[T - 1]
        return torch.tensor(out, dtype=torch.float64).to(dtype=t.dtype, device=t.device).view_as(t)

    def _finish_linear_accum(self):
        """End of a reverse sweep: the partial sums of the fused Linear-sensitivity kernel go into mu (pn_linear_wgrad_finish)."""
        if self._lin is not None:
            self._lin.finish(self, self.adj_p_tensor)

    # ------------------------------------------------------------------ reverse (pa.py:871-890)
    def _step_info(self, k):
        if self._log_override is not None:
            return self._log_override[k]
        tt, hh = ctypes.c_double(), ctypes.c_double()
        check(self._lib.pn_ts_step_log(self._ts, k, ctypes.byref(tt), ctypes.byref(hh)))
        return tt.value, hh.value
