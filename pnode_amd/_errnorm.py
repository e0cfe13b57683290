"""Which weighted error norm a solve hands to its step-size controller (``-ts_adapt_wnormtype 2|infinity``):
the one place that decides.  Every stepper -- the batch and per-sample explicit-RK sweeps, ``ThetaStepper.error_norm``, the ARKIMEX
``error_norm`` and the native step loop -- launches its error estimate and reads it back through the methods here; none of them
calls a backend's ``combine_wrms`` / ``read_enorm`` itself.

  2 (default)  TSErrorWeightedNorm, NORM_2: sqrt(mean(term^2))          pn_rk_combine_wrms / pn_rows_combine_wrms
  infinity     TSErrorWeightedNorm, NORM_INFINITY: max(term), NaN kept  pn_rk_combine_winf / pn_rows_combine_winf

The controller (pn_ts_judge, pn_rows_control) is the same for both: only the number it is given changes."""
import math

import torch

from ._lib import PnError

WINF_METHODS = ("combine_winf", "read_enorm_inf", "rows_combine_winf")


class ErrorNorm(object):
    _winf = False

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
