"""Which weighted error norm a solve hands to its step-size controller (``-ts_adapt_wnormtype 2|infinity``):
the one place that decides.  Every stepper -- the batch and per-sample explicit-RK sweeps, ``ThetaStepper.error_norm``, the ARKIMEX
``error_norm`` and the native step loop -- launches its error estimate and reads it back through the methods here; none of them
calls a backend's ``combine_wrms`` / ``read_enorm`` itself.

  2 (default)  TSErrorWeightedNorm, NORM_2: sqrt(mean(term^2))          pn_rk_combine_wrms / pn_rows_combine_wrms
  infinity     TSErrorWeightedNorm, NORM_INFINITY: max(term), NaN kept  pn_rk_combine_winf / pn_rows_combine_winf

The controller (pn_ts_judge, pn_rows_control) is the same for both: only the number it is given changes.

Against what a term is measured is decided here too: the two scalars of -ts_atol / -ts_rtol, or, after ``setTolerances`` was given a
tensor, one (atol, rtol) pair per component -- then the ``_v`` form of the same entry point is launched
(pn_rk_combine_wrms_v, pn_rk_combine_winf_v, pn_rows_combine_wrms_v, pn_rows_combine_winf_v)."""
import math

import torch

from ._lib import PnError, check

WINF_METHODS = ("combine_winf", "read_enorm_inf", "rows_combine_winf")
VTOL_METHODS = ("combine_wrms_v", "combine_winf_v", "rows_combine_wrms_v", "rows_combine_winf_v")


class ErrorNorm(object):
    _winf = False
    _vtol = None                  # (vatol, vrtol): flat fp64 tensors of one common period on the state's device; None: two scalars
    _tol_spec = (None, None)      # what setTolerances was given, (rtol, atol): None, a float, or an fp64 tensor in the caller's shape

    # ---- per-component tolerances (TSSetTolerances with vectors)
    def setTolerances(self, rtol=None, atol=None):
        """petsc4py's ``ts.setTolerances(rtol, atol)`` on the ``ode.ts`` a user of the reference holds, after ``setupTS``.  Each of
        the two: None (left as it is), a float or 0-d tensor (the scalar of today, overriding -ts_rtol / -ts_atol), a tensor with the
        state's shape, or one with the shape of one sample (``u_tensor.shape[1:]``), repeated over the rows of the batch.  Element e
        of the flattened state is then judged against atol[e % p] + rtol[e % p] * max(|u_e|, |uhat_e|).  Holds for the life of the
        solver; two floats go back to the scalar launches.  Anything unusable is refused by name (PnError)."""
        if self._ops is None:
            raise PnError("setTolerances: call setupTS first (the tolerances are checked against the state it was given)")
        old = self._tol_spec
        spec = []
        for name, new, was in (("rtol", rtol, old[0]), ("atol", atol, old[1])):
            spec.append(was if new is None else self._tol_take(name, new))
        self._tol_spec = tuple(spec)
        scalars = {"atol": self._atol, "rtol": self._rtol}
        try:
            self._tol_apply()
        except Exception:                       # a refused call changes nothing: the two scalars of pn_ts included
            self._tol_spec = old
            for name, x in scalars.items():
                check(self._lib.pn_ts_set_option(self._ts, ("ts_" + name).encode(), repr(x).encode()))
                setattr(self, "_" + name, x)
            self._tol_apply()
            raise
        self._reset_sweep_graphs()

    def _tol_take(self, name, v):
        if isinstance(v, torch.Tensor):
            if v.requires_grad:
                raise PnError("setTolerances: %s requires grad; gradients with respect to the tolerances are not built (pass %s.detach())"
                              % (name, name))
            if not (v.is_floating_point() or v.dtype in (torch.int32, torch.int64)):
                raise PnError("setTolerances: %s must be a real tensor (got %s)" % (name, v.dtype))
            if v.dim() == 0:
                return self._tol_scalar(name, float(v))
            if v.device != self.device:
                raise PnError("setTolerances: %s is on %s, the state on %s; the vectors are read by the error-norm kernels and must "
                              "live on the state's device" % (name, v.device, self.device))
            return v.detach().to(torch.float64).clone()
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise PnError("setTolerances: %s must be None, a float or a tensor (got %s)" % (name, type(v).__name__))
        return self._tol_scalar(name, float(v))

    @staticmethod
    def _tol_scalar(name, x):
        if not math.isfinite(x) or x < 0.0:
            raise PnError("setTolerances: %s must be finite and not negative (got %r)" % (name, x))
        return x

    def _tol_apply(self):
        """From the options' two scalars (self._atol, self._rtol as pn_ts holds them) and what setTolerances asked for to what the
        launches use: two scalars (in pn_ts as well, for the native step loop), or self._vtol.  Called at the end of
        _set_from_options -- so after every setupTS that changed the state or the options -- and by setTolerances."""
        rspec, aspec = self._tol_spec
        shape = tuple(self.tensor_size)
        n = self.n
        B = shape[0] if len(shape) >= 2 else 1
        for name, spec in (("rtol", rspec), ("atol", aspec)):
            if isinstance(spec, float):
                check(self._lib.pn_ts_set_option(self._ts, ("ts_" + name).encode(), repr(spec).encode()))
                setattr(self, "_" + name, spec)
        flat = {}
        for name, spec in (("rtol", rspec), ("atol", aspec)):
            if not isinstance(spec, torch.Tensor):
                continue
            if spec.device != self.device:
                raise PnError("setTolerances: the stored %s is on %s, the state of this setupTS on %s" % (name, spec.device, self.device))
            if tuple(spec.shape) == shape:
                flat[name] = spec.reshape(-1)
            elif len(shape) >= 2 and tuple(spec.shape) == shape[1:]:
                flat[name] = spec.reshape(-1)
            else:
                raise PnError("setTolerances: %s has shape %s; the state has shape %s, so a tolerance tensor has that shape or the shape "
                              "of one sample%s" % (name, tuple(spec.shape), shape, " %s" % (shape[1:],) if len(shape) >= 2 else
                                                   " (none here: a 1-D state has no batch dimension)"))
        if not flat:
            self._vtol = None
            if (rspec is not None or aspec is not None) and self._atol + self._rtol <= 0.0:
                raise PnError("setTolerances: atol + rtol must be positive (got atol %r, rtol %r)" % (self._atol, self._rtol))
            return
        if not getattr(self._ops, "vector_tolerances", False):
            raise PnError("setTolerances: the backend %s has no per-component entry points (vector_tolerances: %s)"
                          % (type(self._ops).__name__, ", ".join(VTOL_METHODS)))
        if self._sample:
            for name, v in flat.items():
                if v.numel() != n // B:
                    raise PnError("setTolerances under -pn_adapt_scope sample: %s has the shape of the whole state %s; the row kernels "
                                  "index a tolerance by column, so give the shape of one sample %s (the rows share it)"
                                  % (name, shape, shape[1:]))
        period = max(v.numel() for v in flat.values())
        vec = {}
        for name, scalar in (("rtol", self._rtol), ("atol", self._atol)):
            v = flat.get(name)
            if v is None:
                v = torch.full((period,), scalar, dtype=torch.float64, device=self.device)
            elif v.numel() != period:                     # one sample beside a whole state: repeated over the rows of the batch
                v = v.reshape(1, -1).expand(period // v.numel(), -1).reshape(-1)
            vec[name] = v.contiguous()
        for name in ("rtol", "atol"):
            v = vec[name]
            if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
                raise PnError("setTolerances: every entry of %s must be finite and not negative" % name)
        if bool(((vec["atol"] + vec["rtol"]) <= 0).any()):
            e = int(torch.nonzero((vec["atol"] + vec["rtol"]) <= 0)[0])
            raise PnError("setTolerances: atol + rtol must be positive for every entry (entry %d of the period of %d has both zero)" % (e, period))
        self._vtol = (vec["atol"], vec["rtol"])

    @property
    def tolerances(self):
        """Against what the error of a step is measured, and by which launches -- a short status string in the style of linear_bwd."""
        if self._ops is None:
            return "not set up"
        if self._vtol is None:
            return "scalar (atol %g, rtol %g)" % (self._atol, self._rtol)

        def span(v):
            lo, hi = float(v.min()), float(v.max())
            return "%g" % lo if lo == hi else "%g \u2026 %g" % (lo, hi)
        loop = ""
        if self._theta is None and not self._sample and self._native and self._adaptive:
            loop = "; forward attempts: Python stage loop"
        return "vector (period %d of n %d; atol %s, rtol %s%s)" % (self._vtol[0].numel(), self.n, span(self._vtol[0]), span(self._vtol[1]), loop)

    def _errnorm_from_options(self):
        """After pn_ts_set_option has seen the options: which norm the solver's pn_ts asks for, and whether the backend has it."""
        self._winf = bool(self._lib.pn_ts_wnorm_infinity(self._ts))
        if self._winf and not getattr(self._ops, "infinity_norm", False):
            raise PnError("-ts_adapt_wnormtype infinity: the backend %s has no infinity-norm entry points (infinity_norm: %s)"
                          % (type(self._ops).__name__, ", ".join(WINF_METHODS)))

    def _wnorm_name(self):
        return "infinity (largest weighted term)" if self._winf else "2 (weighted RMS)"

    # ---- batch scope, theta and ARKIMEX: one norm over the flattened state, finished on the host
    def _err_combine(self, unew, u, Ks, cb, ce):
        """unew = u + sum cb_j K_j (None: `u` already is the new state), err = sum ce_j K_j, and the norm of the solve into the
        backend's result block (read by _err_read)."""
        ops = self._ops
        if self._vtol is not None:
            (ops.combine_winf_v if self._winf else ops.combine_wrms_v)(unew, u, Ks, cb, ce, self._vtol[0], self._vtol[1])
            return
        (ops.combine_winf if self._winf else ops.combine_wrms)(unew, u, Ks, cb, ce, self._atol, self._rtol)

    def _err_read(self):
        """The norm the last _err_combine (or the native step loop) left behind, over this rank's state."""
        ops = self._ops
        return ops.read_enorm_inf() if self._winf else ops.read_enorm()

    def _err_vec_ops(self):
        """The pn_vec_ops table of the native step loop: its rk_combine_wrms member is the combine entry point of the norm."""
        ops = self._ops
        return ops.vec_ops_inf if self._winf else ops.vec_ops

    # ---- sample scope: one norm per row, finished in the launch
    def _err_rows_combine(self, B, d, unew, u, Ks, cb, ce, h, enorm):
        ops = self._ops
        if self._vtol is not None:
            (ops.rows_combine_winf_v if self._winf else ops.rows_combine_wrms_v)(B, d, unew, u, Ks, cb, ce, h, self._vtol[0], self._vtol[1], enorm)
            return
        (ops.rows_combine_winf if self._winf else ops.rows_combine_wrms)(B, d, unew, u, Ks, cb, ce, h, self._atol, self._rtol, enorm)

    # ---- over the ranks of a process group
    def _global_enorm(self, enorm):
        """The norm over the global batch.  2: sqrt(sum_r n_r*enorm_r^2 / sum_r n_r), one all-reduce of two doubles.  infinity: the
        largest of the ranks' norms -- max is associative, so the shards agree on it to the bit whatever the split; one all-reduce
        (MAX) of one double, with a NaN flag beside it, since a backend's MAX need not keep a NaN."""
        import torch.distributed as dist
        if not self._sharded() or not self._pg_global_norm:
            return enorm
        if self._winf:
            nan = math.isnan(enorm)
            v = torch.tensor([0.0 if nan else enorm, 1.0 if nan else 0.0], dtype=torch.float64, device=self.device)
            dist.all_reduce(v, op=dist.ReduceOp.MAX, group=self._pg)
            m, flag = v.tolist()
            return float("nan") if flag > 0.0 else m
        v = torch.tensor([enorm * enorm * self.n, float(self.n)], dtype=torch.float64, device=self.device)
        dist.all_reduce(v, op=dist.ReduceOp.SUM, group=self._pg)
        s, n = v.tolist()
        return (s / n) ** 0.5
