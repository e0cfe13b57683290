"""Drop-in for ``pnode.petsc_adjoint`` on the explicit-RK path, MI355X-native: the surface.

Same surface as the reference (``/root/reference/pnode/petsc_adjoint.py``, "pa.py"): ``ODEPetsc.setupTS / odeint /
odeint_adjoint`` and ``OdeintAdjointMethod`` with the same arguments, argument meaning and error behaviour -- but no
PETSc/petsc4py underneath.  The PETSc TS / TSAdapt / TSAdjoint / TSTrajectory / Vec machinery the reference drives (pa.py:370,
637-656, 766-775, 812-829, 875-878) is replaced by ``libpnode_amd.so`` (``include/pnode_amd.h``): hand-written gfx950 kernels
for all state-vector arithmetic and a C++ host engine for the stepper state machine and the checkpoint schedule.  This file
holds construction, ``setupTS`` and the options, process groups, the argument checks of ``odeint`` and its hand-off to a sweep
(theta / IMEX, per-sample, batch), ``-ts_view``, ``petsc_adjointsolve`` and the autograd entry (pa.py:903-947).  The sweeps are
mixins: the explicit-RK one, forward and reverse, with the callback shells around the user's ``nn.Module`` (pa.py:393-412,
52-82, 341-363) in ``_rk_sweep.py``, the per-sample one in ``_rowsweep.py``, their hipGraph replay in ``_sweepgraphs.py``.

The product path has no CPU fallback: states must live on a HIP device and the shared library must be present, otherwise an
exception is raised.
"""
import contextlib
import ctypes
import sys
import warnings

import torch
import torch.nn as nn

from . import _lib, options
from ._lib import PnError, check  # noqa: F401
from .misc import flat_parameters
from ._errnorm import ErrorNorm
from ._rk_sweep import RKSweep, _mem_now  # noqa: F401
from ._rowsweep import RowSweep
from ._sweepgraphs import SweepGraphs
from ._trajectory import _DiskTrajectory, _Trajectory, _TwoLevelTrajectory  # noqa: F401
from ._vecops import HipVecOps, _KrylovBuffers  # noqa: F401

__all__ = ["ODEPetsc", "OdeintAdjointMethod", "PnError", "PnUnpinnedWarning"]


class PnUnpinnedWarning(RuntimeWarning):
    """Issued once per process and piece when a piece of PETSc's behaviour that is restated here WITHOUT anything
    PETSc-produced to check it against ("parity unpinned") decides the numbers of a solve."""


_UNPINNED_WARNED = set()
_ENV_WARNED = [False]           # the "HIP runtime initialised before import" note of auto graph capture: once per process


def _warn_unpinned(key, what):
    if key in _UNPINNED_WARNED:
        return
    _UNPINNED_WARNED.add(key)
    warnings.warn("pnode_amd: %s -- restated from PETSc's documentation and the literature, not checked against anything "
                  "PETSc produced (no PETSc build and no PETSc-made log exists in the reference): the numbers claim PETSc's "
                  "semantics, not bit-parity with it.  See DESIGN.md section 3 (parity unpinned).  Said once per process."
                  % what, PnUnpinnedWarning, stacklevel=3)


class ODEPetsc(RowSweep, RKSweep, SweepGraphs, ErrorNorm):
    """Explicit-RK neural-ODE solver with discrete adjoint (drop-in for pa.py:366-900).  How its sweeps are launched
    (eagerly, or replayed from hipGraphs) lives in the SweepGraphs mixin, pnode_amd/_sweepgraphs.py."""

    def __init__(self, backend=None):
        self._lib = _lib.load()
        self._backend_cls = backend if backend is not None else HipVecOps
        self._ts = ctypes.c_void_p(self._lib.pn_ts_create())
        self.n = 0
        self.tensor_size = None
        self.tensor_dtype = None
        self.device = None
        self.adj_u = []
        self.adj_p = []
        self.mass = None
        self.funcIM = None
        self.funcEX = None
        self.flat_params = None
        self.npIM = self.npEX = self.np = None
        self.imex = None
        self.use_dlpack = True
        self.linear_solver = None
        self.matrixfree_jacobian = True
        self.step_size = 0.01
        self.enable_adjoint = True
        self._traj = None
        self._tmode = None
        self._ops = None
        self._nsteps = 0
        self._tapes = None
        self._init_sweep_graphs()
        self._dense = False            # -pn_output_times interpolate
        self._dense_active = False     # ... and the last forward solve had output times inside its steps
        self._lin = None               # engine-side parameter sensitivities of func's nn.Linear layers (_lineargrad.py)
        self._pend_mixed = False
        self._sg = None                # the per-evaluation hipGraphs the sweep in progress replays (pnode_amd/_stagegraphs.py)
        self._unit_capture = False
        self._lin_sig = None
        self._fwd = None               # func's Linear -> Tanh pairs as one launch in the solver's own evaluations (_linearfwd.py)
        self._fwd_sig = None
        self._theta = None
        self._tgrad = False            # the solve in progress differentiates with respect to t
        self._tg = None                # ... and the reverse sweep in progress accumulates dL/dt (RKSweep._tg_begin)
        self._tg_warned = False
        self._theta_method = None
        self._imex_built = False
        self._paramsI = self._paramsE = self._pnamesI = self._pnamesE = ()
        self._options_sig = None
        self._view = False
        self._rtapes = None
        self._trace = False
        self._pg_enabled = False
        self._pg = None
        self._pg_average = True
        self._pg_global_norm = True
        self.nfe_forward = 0      # f evaluations in forward sweeps (NFE-F of the reference's examples)
        self.nfe_backward = 0     # f evaluations (each followed by a VJP) in reverse sweeps (NFE-B)

    def __del__(self):
        try:
            if self._lin is not None:
                self._lin.remove()             # the forward hooks on func's Linear layers go with the solver
        except Exception:
            pass
        try:
            self._lib.pn_ts_destroy(self._ts)
        except Exception:
            pass

    # ------------------------------------------------------------------ introspection
    @property
    def num_steps(self):
        """Accepted time steps of the last forward solve."""
        return self._nsteps

    @property
    def num_rejections(self):
        """Rejected step attempts of the last forward solve (adaptive schemes)."""
        return int(self._lib.pn_ts_rejections(self._ts))

    def step_log(self):
        """[(t_n, h_n)] of the accepted steps of the last forward solve."""
        return [self._step_info(k) for k in range(self._nsteps)]

    # ------------------------------------------------------------------ multi-GPU
    def setProcessGroup(self, group=None, average=True, global_error_norm=True, enabled=True):
        """Shard the batch of trajectories over the ranks of a ``torch.distributed`` group
        (one process per GPU; backend "nccl" is RCCL over xGMI).  Every rank integrates its own
        contiguous batch shard with replicated parameters; the only data-path exchange is ONE
        all-reduce of the flat parameter-gradient buffer per backward.  ``average`` divides by
        the world size (loss = mean over the global batch).  With an adaptive method
        ``global_error_norm`` additionally all-reduces one scalar (sum of squares; under
        ``-ts_adapt_wnormtype infinity`` the maximum, _errnorm.py) per step
        attempt so that every rank takes the reference's step sequence, whose WRMS norm spans
        the whole flattened batch; turning it off gives per-shard controllers (not parity).
        The reference has no counterpart (it is single-process, pa.py:367 COMM_SELF)."""
        self._pg_enabled = enabled
        self._pg = group
        self._pg_average = average
        self._pg_global_norm = global_error_norm

    def _sharded(self):
        """True when a process group is attached: the collectives are then issued whatever the group's
        size (a one-rank group reduces to itself -- that is how the RCCL path is exercised on one GPU)."""
        import torch.distributed as dist
        return bool(self._pg_enabled and dist.is_available() and dist.is_initialized())

    def _world(self):
        import torch.distributed as dist
        return dist.get_world_size(self._pg) if self._sharded() else 1

    def _allreduce_adj_p(self, tgrad=False):
        """mu summed (and averaged) over the ranks; with `tgrad` (this backward computes dL/dt) the per-rank dL/dt accumulators too."""
        import torch.distributed as dist
        tg = self._tg["acc"] if (tgrad and self._tg is not None) else None
        if not self._sharded() or (self.np == 0 and tg is None):
            return
        w = self._world()
        if tg is not None and (self.np == 0 or self.adj_p_tensor.dtype == tg.dtype):
            # the per-rank partial dL/dt joins the all-reduce of mu (fp64 states); fp32 ones keep it in double, beside
            v = torch.cat([self.adj_p_tensor, tg]) if self.np else tg
            dist.all_reduce(v, op=dist.ReduceOp.SUM, group=self._pg)
            if self.np:
                self.adj_p_tensor.copy_(v[: self.np])
                tg.copy_(v[self.np:])
            tg_done = True
        else:
            dist.all_reduce(self.adj_p_tensor, op=dist.ReduceOp.SUM, group=self._pg)
            tg_done = tg is None
        if not tg_done:
            dist.all_reduce(tg, op=dist.ReduceOp.SUM, group=self._pg)
        if self._pg_average and w > 1:
            if self.np:
                self.adj_p_tensor.mul_(1.0 / w)
            if tg is not None:
                tg.mul_(1.0 / w)

    # ------------------------------------------------------------------ setup (pa.py:534-775)
    def setupTS(self, u_tensor, func, step_size=0.01, enable_adjoint=True, implicit_form=False,
                use_dlpack=True, method="dopri5", mass=None, imex_form=False, func2=None,
                batch_size=1, linear_solver="petsc", fixed_jacobian=False, matrixfree_jacobian=True,
                fixed_jacobian_across_solves=None):
        """Set up the solver before it is used.  Arguments as in pa.py:551-584.

        ``u_tensor`` only donates shape, dtype and device.  ``step_size`` is a float or a list
        (per-step sizes).  ``use_dlpack``, ``batch_size``, ``linear_solver``,
        ``fixed_jacobian`` and ``matrixfree_jacobian`` are accepted and have no effect on the
        explicit path (there is one zero-copy mode and no linear solve); on the IMEX path
        ``linear_solver="torch"`` selects the direct stage solve and ``fixed_jacobian=True`` keeps its
        factors across solves when funcIM has no trainable parameter.  As in the reference,
        ``method`` is applied only when shape, dtype or device change (pa.py:627-656), and
        command-line options (``pnode_amd.init(argv)``) override it (pa.py:775).
        """
        if imex_form and func2 is None:
            raise ValueError("func2 must be provided to enable imex_form=True")
        if fixed_jacobian_across_solves is not None:
            # examples-sinode/KS/KS.py:494,516 still pass the keyword's earlier name
            fixed_jacobian = bool(fixed_jacobian_across_solves)
        from .theta import THETA_METHODS
        theta_method = implicit_form and not imex_form and method in THETA_METHODS
        imex_method = bool(imex_form) and method == "imex"
        if (implicit_form or imex_form or method in ("beuler", "cn", "imex")) and not (theta_method or imex_method):
            raise NotImplementedError(
                "pnode_amd implements the explicit-RK path (euler/midpoint/rk2/bosh3/rk4/dopri5), the implicit "
                "theta methods (implicit_form=True with method 'beuler' or 'cn') and IMEX (imex_form=True with "
                "method 'imex'); other combinations are not built (DESIGN.md section 8)")
        self.imex = imex_form
        self.linear_solver = linear_solver
        self.fixed_jacobian = fixed_jacobian
        self.matrixfree_jacobian = matrixfree_jacobian
        tensor_dtype = u_tensor.dtype
        tensor_size = u_tensor.size()
        device = u_tensor.device
        n = u_tensor.numel()
        if self.funcIM is not func or (imex_form and self.funcEX is not func2) or bool(imex_form) != bool(self._imex_built):
            # pa.py:600-621 -- IMEX: func is treated implicitly, func2 explicitly, flat parameters
            # = [func's, func2's]; otherwise func2 is ignored
            self._imex_built = bool(imex_form)
            self.funcIM = func
            self.funcEX = func2 if imex_form else func
            def trainable(f):
                if not isinstance(f, nn.Module):
                    return (), ()
                return (tuple(p for p in f.parameters() if p.requires_grad),
                        tuple(n for n, p in f.named_parameters() if p.requires_grad))
            self._paramsI, self._pnamesI = trainable(self.funcIM)
            self._paramsE, self._pnamesE = trainable(self.funcEX)
            self._params = self._paramsI + self._paramsE if imex_form else self._paramsE
            # The reference routes dL/dtheta through a cat of parameter views (pa.py:618-620).
            # Here the parameters themselves are inputs of the autograd Function (its `*args`),
            # and flat_params is a detached copy kept for its size/order only: a live cat graph
            # pins the parameters' AccumulateGrad nodes to the stream it was built on, which
            # breaks hipGraph capture of the reverse sweep.
            with torch.no_grad():
                self.flat_params = flat_parameters(self._params)
            self.np = self.flat_params.numel()
            self.npIM = sum(p.numel() for p in self._paramsI) if imex_form else self.np
            self.npEX = self.np - self.npIM if imex_form else self.np
            self._poff, off = [], 0
            for p in self._params:
                self._poff.append(off)
                off += p.numel()
            self._plen = [p.numel() for p in self._params]
            nI = len(self._paramsI) if imex_form else 0
            self._poffI, self._plenI = self._poff[:nI], self._plen[:nI]
            self._poffE, self._plenE = self._poff[nI:], self._plen[nI:]
            self.adj_p_tensor = None
            self._reset_sweep_graphs(new_func=True)
        if self.mass is not mass:
            self.mass = mass
        if tensor_size != self.tensor_size or tensor_dtype != self.tensor_dtype or device != self.device:
            self._ops = self._backend_cls(device, tensor_dtype, n)
            self.tensor_size = tensor_size
            self.tensor_dtype = tensor_dtype
            self.device = device
            self.use_dlpack = use_dlpack
            self.n = n
            self._npad = (n + 63) // 64 * 64
            check(self._lib.pn_ts_set_rk_type(self._ts, self._lib.pn_method_to_rk_type(str(method).encode())))
            self._theta_method = method if theta_method else ("imex" if imex_method else None)   # on rebuild only
            self.adj_u_tensor = None
            self.adj_p_tensor = None
            self._traj = None
            self._work = {}
            self._reset_sweep_graphs()
        self.step_size = step_size
        self.enable_adjoint = enable_adjoint
        if not enable_adjoint:
            self._traj = None          # ts.removeTrajectory() (pa.py:773-774)
        # ts.setFromOptions() (pa.py:775).  Callers such as train-Cifar10.py:121-139 call setupTS on
        # every forward: when neither the tableau choice nor the options database changed since
        # the last call this is a dictionary comparison, not a re-parse.
        sig = (options.get_all(), self._theta_method, id(self._ops))
        if sig != self._options_sig:
            self._set_from_options()
            self._theta = None
            self._reset_sweep_graphs()  # captured sweeps belong to the scheme and modes they were captured with
            # -ts_type on the command line overrides the `method` keyword, as ts.setFromOptions() does
            # (README.md:89: "-ts_type cn will choose the Crank-Nicolson methods")
            ts_type = str(options.get_all().get("ts_type", ""))
            stepper = self._theta_method
            if ts_type in ("beuler", "cn", "theta") and stepper != "imex":
                stepper = ts_type
            elif ts_type == "rk" and stepper != "imex":
                stepper = None
            elif ts_type == "arkimex" and stepper != "imex":
                raise PnError("-ts_type arkimex needs the IMEX set-up (setupTS(..., imex_form=True, method='imex', func2=...))")
            elif ts_type in ("beuler", "cn", "theta", "rk") and stepper == "imex":
                raise PnError("-ts_type %s cannot override an IMEX set-up (two functions were given)" % ts_type)
            self._stepper_kind = stepper
            if self._dense:
                if stepper:
                    raise PnError("-pn_output_times interpolate is built for the explicit RK tableaus 3bs (bosh3), 4 (rk4) and 5dp "
                                  "(dopri5); the theta / IMEX steppers take matched output times only")
                self._dense_order, P = _lib.ts_tableau_dense(self._ts)        # PnError for a tableau without an extension
                self._dense_P = P[: self._s]
                self._dense_cols = [j for j in range(self._s) if any(v != 0.0 for v in P[j])]
            adapt_wanted = str(options.get_all().get("ts_adapt_type", "basic")) != "none"
            if stepper == "imex":
                from .arkimex import ArkimexStepper
                self._theta = ArkimexStepper(self, options.get_all())
                has_embed = self._theta.embedded() is not None
                check(self._lib.pn_ts_set_scheme(self._ts, self._theta.tab["adapt_order"], 1 if has_embed else 0))
                if adapt_wanted and not has_embed:
                    warnings.warn("pnode_amd: ARKIMEX type %s has no embedded weights here and takes the fixed steps of "
                                  "step_size; PETSc adapts unless -ts_adapt_type none is given (every IMEX run of the "
                                  "reference gives it).  Pass -ts_adapt_type none to state that explicitly, or use type "
                                  "3, 4, 5 or 1bee." % self._theta.name, RuntimeWarning)
                self._adaptive = bool(self._lib.pn_ts_is_adaptive(self._ts))
                if self._theta.name in ("l2", "2c", "2d", "2e"):
                    _warn_unpinned("arkimex_table_" + self._theta.name,
                                   "ARKIMEX type %s: the identification of this table with PETSc's type of that name "
                                   "(l2) / the free entries of its explicit part (2c, 2d, 2e) are" % self._theta.name)
                if self._adaptive:
                    _warn_unpinned("arkimex_adapt", "adaptive ARKIMEX steps (TSAdapt basic on the embedded pair; embedded "
                                   "weights, controller constants and step rejection are")
            elif stepper:
                from .theta import ThetaStepper
                self._theta = ThetaStepper(self, stepper, options.get_all())
                # TSCreate_Theta sets the TS's default adapt type to NONE: beuler / cn take the fixed steps of
                # step_size unless `-ts_adapt_type basic` is given explicitly (the reference's spiral_unstable.py
                # and ode_demo_petsc.py give no adapt option and run cn / beuler with fixed steps).  With it, PETSc
                # estimates the local truncation error from the last three solutions and the controller uses
                # order 2 (see ThetaStepper.error_norm).
                explicit_basic = str(options.get_all().get("ts_adapt_type", "")) == "basic"
                check(self._lib.pn_ts_set_scheme(self._ts, 2, 1 if explicit_basic else 0))
                self._adaptive = bool(self._lib.pn_ts_is_adaptive(self._ts))
                if self._adaptive:
                    _warn_unpinned("theta_adapt", "adaptive beuler / cn steps (-ts_adapt_type basic: the three-solution local "
                                   "truncation error estimate of TSEvaluateWLTE_Theta and its controller order are")
            else:
                check(self._lib.pn_ts_set_scheme(self._ts, 0, 0))          # the RK tableau drives the controller
            self._options_sig = sig
        if self._sample:
            self._rows_refusals()
        self._setup_linear_grads()

    def _set_from_options(self):
        """ts.setFromOptions() (pa.py:775) for the option subset of this path."""
        db = options.get_all()
        self._monitor = "ts_monitor" in db
        self._view = "ts_view" in db
        if "log_view" in db and self.device.type == "cuda":
            from . import logview
            logview.enable()
        # not a PETSc option: bracket the sweeps with roctx ranges (visible to rocprofv3 --marker-trace)
        self._trace = self.device.type == "cuda" and options.truthy(db.get("pn_trace"), False) if "pn_trace" in db else False
        # not a PETSc option: ONE switch that takes back every default of this package that a user of the reference
        # could observe (all of them leave the gradients bit-identical):
        #   * stage tapes are not retained (-pn_trajectory_retain_graph 0): func is re-evaluated inside every stage VJP
        #     of the reverse sweep, as RHSJacShell.multTranspose does (pa.py:66-74), so funcs that count their calls
        #     (NFE-B of the reference's drivers, examples-pnode/spiral_unstable.py:326-347) read what they read there;
        #   * PETSc's trajectory default stays solution-only whatever fits in HBM (no automatic stage keeping), and a
        #     reversed step is recomputed WHOLE, last stage derivative included, as TSTrajectory's TSStep does;
        #   * the steps of an output interval are counted with the reference's +-1e-5 / 1e-3 window (-pn_span_count
        #     reference, pa.py:527-532);
        #   * the Newton-Krylov solves launch func eagerly (-pn_krylov_graph 0): its side effects happen at every call.
        # Each of these can still be set on its own; an explicit option wins over the switch.
        self._ref_defaults = options.truthy(db.get("pn_reference_defaults"), False) if "pn_reference_defaults" in db else False
        self._solution_only = options.truthy(db.get("ts_trajectory_solution_only"), True)
        # option not given: PETSc's default (states only, stages recomputed) unless everything fits easily, see _pick_traj_mode
        self._solution_only_auto = "ts_trajectory_solution_only" not in db and not self._ref_defaults
        ram = int(float(db["ts_trajectory_max_cps_ram"])) if db.get("ts_trajectory_max_cps_ram", "") != "" else 0
        disk = int(float(db["ts_trajectory_max_cps_disk"])) if db.get("ts_trajectory_max_cps_disk", "") != "" else 0
        if ram < 0 or disk < 0:
            raise PnError("-ts_trajectory_max_cps_ram / -ts_trajectory_max_cps_disk must not be negative")
        # PETSc's two levels: at most `ram` checkpoints in memory (HBM here) and `disk` more in files; one scheduler places the
        # ram + disk of them (_TwoLevelTrajectory).  Only -ts_trajectory_max_cps_disk: the bounded set lives in files.
        self._max_cps = ram + disk
        self._max_cps_ram, self._max_cps_disk = ram, disk
        # -ts_trajectory_type: "memory" = HBM (the default here; PETSc's default is "basic" = one file per checkpoint,
        # which is what "basic" selects here too); PETSc's other types are not built and are refused, not ignored
        ttype = str(db.get("ts_trajectory_type", "memory"))
        if ttype not in ("memory", "basic"):
            raise PnError("-ts_trajectory_type %s is not implemented by pnode_amd (memory: checkpoints in HBM; basic: one file "
                          "per checkpoint under -ts_trajectory_dirname)" % ttype)
        self._traj_disk = ttype == "basic" or disk > 0
        self._traj_all_on_disk = ttype == "basic"          # -ts_trajectory_type basic: every checkpoint is a file, whatever the budgets
        self._traj_dirname = str(db.get("ts_trajectory_dirname", "SA-data"))
        self._traj_keep = options.truthy(db.get("ts_trajectory_keep_files"), False) if "ts_trajectory_keep_files" in db else False
        # not a PETSc option.  With store-all checkpoints (-ts_trajectory_solution_only 0) the forward sweep can
        # also keep every stage's autograd tape, so that the reverse sweep runs only the backward half of each
        # stage VJP instead of re-evaluating f first (pa.py:66-68 re-evaluates).  Same bits either way.
        #   auto (default): tapes are kept while they fit in half of the HBM that is free when the sweep starts
        #   1: always   0: never (the reference's recompute)
        rg = str(db.get("pn_trajectory_retain_graph", "0" if self._ref_defaults else "auto"))
        self._retain_graph = 2 if rg == "auto" else (1 if options.truthy(rg, False) else 0)
        # not a PETSc option: how the steps of an output interval are counted (see _span_post_step)
        self._span_count_reference = str(db.get("pn_span_count", "reference" if self._ref_defaults else "exact")) == "reference"
        self._accum_mode = str(db.get("pn_param_accum", "batch"))
        if self._accum_mode not in ("batch", "step", "stage"):
            raise PnError("-pn_param_accum must be batch, step or stage")
        self._accum_sources = max(1, min(32, int(float(db.get("pn_param_accum_sources", 32)))))
        # not a PETSc option: who walks the tableau.  native (default): one C++ entry point per step attempt / reversed step
        # (pn_rk_attempt, pn_rk_adjoint_step -- PETSc's C loops behind ts.solve / ts.adjointSolve, pa.py:829, 878) that calls
        # back only for func and its VJP; python: the stage loop of rounds 1-3, one ctypes call per launch.  Same launches,
        # same coefficients, same bits.
        sl = str(db.get("pn_step_loop", "native"))
        if sl not in ("native", "python"):
            raise PnError("-pn_step_loop must be native or python")
        self._native = sl == "native" and bool(getattr(self._ops, "native_steps", False))
        # not a PETSc option: after GRAPH_WARMUP_CALLS eager calls with the same shapes/times,
        # capture the whole forward sweep and the whole reverse sweep as two hipGraphs and
        # replay them (fixed-step only; func must be capturable: no host-side data dependence)
        #   auto (the default on a HIP device; off under -pn_reference_defaults): explicit fixed-step RK sweeps only, and only
        #        when it is safe and pays -- see _graph_entry / _auto_capture_forward: plain call counters of func keep counting
        #        (their increments are learnt in the warm-up calls), any other Python-side change during a sweep keeps the solver
        #        eager, the first replay of each sweep is compared with the eager sweep of the same call, and replay must not
        #        be slower than the eager launches it replaces
        #   1: always (every capturable stepper; a failure to capture warns and falls back)      0: never
        gco = str(db.get("pn_graph_capture", "0" if self._ref_defaults else "auto"))
        self._graph_mode = 2 if gco == "auto" else (1 if options.truthy(gco, False) else 0)
        self._graph_status = "eager (-pn_graph_capture 0)" if self._graph_mode == 0 else "eager (warming up)"
        self._auto_veto = None
        # not a PETSc option: in auto mode every N-th replayed call of a captured pair is ALSO run eagerly and compared, as
        # the call that captured it was (0: never).  Catches state of func that the capture guard cannot see.
        self._revalidate_every = int(float(db.get("pn_graph_revalidate", self.GRAPH_REVALIDATE_EVERY)))
        if self._revalidate_every < 0:
            raise PnError("-pn_graph_revalidate must not be negative")
        # not a PETSc option: how the output times t[1:-1] are produced
        #   match (default): every output time ends a step (the reference's TSSetTimeSpan / MATCHSTEP)
        #   interpolate: the stepper sees [t[0], t[-1]] only; outputs inside a step come from the tableau's continuous extension
        om = str(db.get("pn_output_times", "match"))
        if om not in ("match", "interpolate"):
            raise PnError("-pn_output_times must be match or interpolate (got '%s')" % om)
        self._dense = om == "interpolate"
        self._dense_P = None
        # not a PETSc option: what one step-size controller spans
        #   batch (default): the whole flattened state -- one WRMS norm, one step size, the reference's behaviour
        #   sample: every row of the state's first dimension has its own norm, time, step size and accept / reject
        sc = str(db.get("pn_adapt_scope", "batch"))
        if sc not in ("batch", "sample"):
            raise PnError("-pn_adapt_scope must be batch or sample (got '%s')" % sc)
        self._sample = sc == "sample"
        if self._sample:
            self._graph_status = "eager (-pn_adapt_scope sample: the rounds of a per-sample solve are launched eagerly)"
        self._rows_compact_from_options(db)
        for key, val in db.items():
            if key.startswith("ts_trajectory") or key in ("ts_monitor", "ts_view") or key.startswith("pn_"):
                continue
            if key == "ts_type" and str(val) in ("beuler", "cn", "theta", "arkimex"):
                continue
            if key.startswith("ts_arkimex") or key.startswith("ts_theta"):
                continue
            if key.startswith("ts_"):
                try:
                    check(self._lib.pn_ts_set_option(self._ts, key.encode(), str(val).encode()))
                except PnError as exc:
                    raise PnError("PETSc option -%s %s is not implemented by pnode_amd (%s). Implemented: -ts_type, -ts_rk_type, "
                                  "-ts_adapt_type none|basic, -ts_rtol, -ts_atol, -ts_max_steps, -ts_max_reject, -ts_adapt_safety, "
                                  "-ts_adapt_reject_safety, -ts_adapt_clip, -ts_adapt_dt_min, -ts_adapt_dt_max, -ts_adapt_wnormtype 2|infinity, "
                                  "-ts_arkimex_type, "
                                  "-ts_trajectory_*, -ts_monitor, -ts_view, -snes_*, -ksp_*, -log_view; an option that could change "
                                  "the numbers is refused rather than ignored" % (key, val, exc)) from None
        tab = _lib.Tableau()
        check(self._lib.pn_ts_get_tableau(self._ts, ctypes.byref(tab)))
        s = tab.s
        self._s = s
        self._fsal = bool(tab.fsal)
        self._s_eff = s - 1 if self._fsal else s      # stages whose adjoint is not structurally zero
        self._A = [[tab.A[i][j] for j in range(s)] for i in range(s)]
        self._b = [tab.b[j] for j in range(s)]
        self._c = [tab.c[j] for j in range(s)]
        self._e = [tab.bembed[j] - tab.b[j] for j in range(s)]
        self._plans = {}
        self._adaptive = bool(self._lib.pn_ts_is_adaptive(self._ts))
        a, r = ctypes.c_double(), ctypes.c_double()
        check(self._lib.pn_ts_get_tolerances(self._ts, ctypes.byref(a), ctypes.byref(r)))
        self._atol, self._rtol = a.value, r.value
        self._errnorm_from_options()          # -ts_adapt_wnormtype: which norm, and whether the backend has it
        self._tol_apply()                     # what setTolerances asked for holds across set-ups (PnError where it no longer fits)
        # budgeted checkpoints with -ts_trajectory_solution_only 0: a checkpoint holds the stage values
        # of its step as well (PETSc's checkpoints do), so reversing a checkpointed step recomputes nothing
        self._budget_stages = self._max_cps > 0 and not self._solution_only
        if self._max_cps > 0:
            self._traj_mode = _lib.PN_TRAJ_BUDGET
        elif self._solution_only:
            self._traj_mode = _lib.PN_TRAJ_SOLUTION
        else:
            self._traj_mode = _lib.PN_TRAJ_ALL

    def _new_trajectory(self, vecs, mode):
        """TSTrajectory of the coming forward sweep: HBM slabs, or files for -ts_trajectory_type basic (every placement:
        all steps, or the bounded set of -ts_trajectory_max_cps_ram)."""
        if self._max_cps_disk > 0 and self._max_cps_ram > 0 and mode == _lib.PN_TRAJ_BUDGET and not self._traj_all_on_disk:
            return _TwoLevelTrajectory(self._lib, self._ops, self.n, vecs, mode, self._max_cps, self._traj_dirname, self._traj_keep,
                                       self._max_cps_ram)
        if self._traj_disk:
            return _DiskTrajectory(self._lib, self._ops, self.n, vecs, mode, self._max_cps, self._traj_dirname, self._traj_keep)
        return _Trajectory(self._lib, self._ops, self.n, vecs, mode, self._max_cps)

    # ------------------------------------------------------------------ helpers
    def _buf(self, name):
        b = self._work.get(name)
        if b is None:
            b = self._ops.empty(self._npad)
            self._work[name] = b
        return b

    def _shaped(self, flat):
        return flat[: self.n].view(self.tensor_size)

    # ------------------------------------------------------------------ forward (pa.py:777-869)
    def odeint(self, u0, t):
        """Solve du/dt = func(t, u), u(t[0]) = u0; returns the states at the times `t`
        (first dimension), or, when `t` has one element, integrates [0, t[0]] (pa.py:818-820)."""
        self._tgrad = False
        return self._odeint(u0, t, self.enable_adjoint)

    @contextlib.contextmanager
    def _device_guard(self):
        """The device entry points launch on the calling thread's current HIP device: make it the solver's device for the
        duration of a sweep, and pin the backend's launches to the stream that is current now (nothing to do for the CPU test
        stand-in, nor for a backend without a pinned stream)."""
        if self.device is None or self.device.type != "cuda":
            yield
            return
        with torch.cuda.device(self.device):
            ops = self._ops
            if not hasattr(ops, "_pinned_stream"):
                yield
                return
            prev, ops._pinned_stream = ops._pinned_stream, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            try:
                yield
            finally:
                ops._pinned_stream = prev

    def _traced(self, name, fn, *args):
        """fn(*args) on the solver's device; under -pn_trace inside an nvtx range (a roctx range on ROCm, visible to
        rocprofv3 --marker-trace)."""
        with self._device_guard(), (torch.cuda.nvtx.range(name) if self._trace else contextlib.nullcontext()):
            return fn(*args)

    def _odeint(self, u0, t, save):
        return self._traced("pnode_amd.forward_sweep", self._odeint_impl, u0, t, save)

    def _odeint_impl(self, u0, t, save):
        if self._ops is None:
            raise RuntimeError("setupTS must be called before odeint")
        if u0.size() != self.tensor_size or u0.dtype != self.tensor_dtype or u0.device != self.device:
            raise ValueError("u0 does not match the tensor given to setupTS (shape, dtype, device)")
        self._dense_active = False
        if self._theta is not None:
            return self._theta.odeint(u0, t, save)
        if self._sample:
            return self._rows_odeint(u0, t, save)
        return self._rk_odeint(u0, t, save)

    def _ts_view(self):
        """-ts_view: the solver's settings and counters after a solve (PETSc prints its TS object there)."""
        modes = {_lib.PN_TRAJ_ALL: "every step, with stage values", _lib.PN_TRAJ_SOLUTION: "every step, solution only",
                 _lib.PN_TRAJ_BUDGET: "at most %d checkpoints (%s)" % (self._max_cps, "with stage values" if self._budget_stages else "solution only")}
        tab = _lib.Tableau()
        check(self._lib.pn_ts_get_tableau(self._ts, ctypes.byref(tab)))
        print("TS Object (pnode_amd): type rk, order %d, %d stages%s%s"
              % (tab.order, tab.s, ", first same as last" if tab.fsal else "", ", embedded error estimate" if tab.has_embed else ""))
        print("  adapt: %s%s" % ("basic, atol %g rtol %g, error norm %s" % (self._atol, self._rtol, self._wnorm_name()) if self._adaptive
                                 else "none (fixed steps)",
                                 "; final time matched exactly (MATCHSTEP)"))
        print("  state: %s %s on %s;  trainable parameters: %d" % (tuple(self.tensor_size), str(self.tensor_dtype).replace("torch.", ""), self.device, self.np))
        print("  tolerances: %s" % self.tolerances)
        print("  launches: %s;  step loop: %s" % (self._graph_status, "C++ (pn_rk_attempt / pn_rk_adjoint_step)" if self._native else "Python"))
        print("  output times: %s" % ("interpolate (continuous extension of order %d; the steps are those of the end points alone)"
                                      % self._dense_order if self._dense else "match (a step ends on every output time)"))
        print("  total number of time steps=%d, rejected=%d;  trajectory: %s"
              % (self._nsteps, self._lib.pn_ts_rejections(self._ts), modes[self._tmode] if self._traj is not None else "not saved"))

    def petsc_adjointsolve(self, t, i=1):
        """Reverse one output interval (pa.py:871-890): all steps when `t` has one element,
        else the ``cur_sol_steps[i]`` steps that led to output time i."""
        if self._sample:
            raise PnError("petsc_adjointsolve by output interval is not available under -pn_adapt_scope sample: the rows reach the "
                          "output times in different rounds (odeint_adjoint's backward covers all outputs)")
        if self._dense and t.shape[0] > 1:
            raise PnError("petsc_adjointsolve by output interval is not available under -pn_output_times interpolate: the output "
                          "times no longer end steps (odeint_adjoint's backward covers all outputs)")
        self._adjoint_steps(self._nsteps if t.shape[0] == 1 else self.cur_sol_steps[i], None)
        self._flush_param_accum()
        self._finish_linear_accum()
        return self._shaped(self.adj_u_flat), self.adj_p_tensor

    # ------------------------------------------------------------------ autograd entry (pa.py:892-900)
    def odeint_adjoint(self, y0, t):
        if not isinstance(self.funcIM, nn.Module):
            raise ValueError("func is required to be an instance of nn.Module.")
        # inside Function.forward grad mode is always off, so note here whether a backward can follow
        self._grad_mode = torch.is_grad_enabled()
        return OdeintAdjointMethod.apply(y0, t, self.flat_params, self, *self._params)


class OdeintAdjointMethod(torch.autograd.Function):
    """pa.py:903-947.  Forward: solve under no_grad.  Backward: seed lambda with dL/dy(t_T),
    reverse the output intervals newest first, adding dL/dy(t_{i-1}) after each one."""

    @staticmethod
    def forward(ctx, y0, t, flat_params, ode, *args):
        ctx.ode = ode
        # dL/dt: explicit RK only; -pn_reference_defaults keeps the reference's None (pa.py:947)
        tg = bool(ctx.needs_input_grad[1]) and ode._tgrad_supported()
        need = ode.enable_adjoint and ode._grad_mode and (ctx.needs_input_grad[0] or any(ctx.needs_input_grad[4:]) or tg)
        ode._tgrad = ctx.tgrad = bool(tg and need)
        with torch.no_grad():
            ans, e, warm = ode._sweep_forward(y0, t, need)
        ctx.graph_entry = e
        ctx.warm_entry = warm
        if "pnode_amd.logview" in sys.modules:
            sys.modules["pnode_amd.logview"].note_forward(ode)
        ctx.save_for_backward(t, flat_params, ans)
        return ans

    @staticmethod
    def backward(ctx, *grad_output):
        t, flat_params, ans = ctx.saved_tensors
        ode = ctx.ode
        T = ans.shape[0]
        g = grad_output[0]
        if g.dtype != ode.tensor_dtype:
            g = g.to(ode.tensor_dtype)
        g = g.contiguous().view(T, -1)
        with torch.no_grad():
            ode._tgrad = ctx.tgrad
            try:
                ode._sweep_backward(ctx.graph_entry, getattr(ctx, "warm_entry", None), g, T)
                ode._allreduce_adj_p(tgrad=ctx.tgrad)
                adj_t = ode._tg_finish(t) if ctx.tgrad else None
            finally:
                ode._tg = None             # (a backward that raised leaves no accumulators behind for a later one)
            if "pnode_amd.logview" in sys.modules:
                sys.modules["pnode_amd.logview"].note_backward(ode)
            adj_u = ode._shaped(ode.adj_u_flat).detach().clone()
            adj_p = ode.adj_p_tensor.detach().clone()
            gparams = tuple(adj_p[o:o + l].view_as(p).to(p.dtype) for p, o, l in zip(ode._params, ode._poff, ode._plen))
        return (adj_u, adj_t, None, None) + gparams
