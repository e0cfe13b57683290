"""The device entry points of ``include/pnode_amd.h`` as methods on tensors: ``HipVecOps`` (what ODEPetsc calls ``self._ops``;
the CPU-only test-suite injects ``tests/_cpu_vecops.py`` in its place) and the buffers of the device-resident GMRES.  Each method
names the C entry point it wraps; what that entry point replaces in PETSc is in the header."""
import contextlib
import ctypes
import warnings

import torch
import torch.nn as nn  # noqa: F401

from . import _lib, options
from ._lib import PnError, check  # noqa: F401


class HipVecOps(object):
    """Device entry points of the C ABI over flat torch tensors on one HIP device."""

    def __init__(self, device, dtype, n):
        if device.type != "cuda":
            raise RuntimeError(
                "pnode_amd runs on MI355X HIP devices only (got a %s tensor); there is no CPU path" % device.type)
        self.lib = _lib.load()
        self.device, self.dtype, self.n = device, dtype, n
        self.code = _lib.dtype_code(dtype)
        self.work = None
        self.dots_work = None
        self._err_host = self._err_dev = None
        self._pinned_stream = None
        self._seg_cache = {}
        self._ptr_buf = (ctypes.c_void_p * 16)()
        self._colsum_work = None

    def __del__(self):
        try:
            for h in (self._err_host, getattr(self, "_dots_host", None)):
                if h is not None and h.value:
                    self.lib.pn_pinned_free(h)
        except Exception:
            pass

    def stream(self):
        """The calling thread's current HIP stream (pinned for the duration of a sweep: looking it
        up costs more host time than a launch)."""
        st = self._pinned_stream           # (a c_void_p holding 0 -- the default stream -- is falsy: compare with None)
        return st if st is not None else ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def empty(self, *shape):
        return torch.empty(*shape, dtype=self.dtype, device=self.device)

    def _ptrs(self, tensors):
        """Device pointers of `tensors` as a C array.  One reusable array: the entry points copy what they need
        before they return, and building a ctypes array per launch costs more host time than the launch."""
        buf = self._ptr_buf
        k = 0
        for t in tensors:
            buf[k] = t.data_ptr()
            k += 1
        return buf

    @staticmethod
    def _dbl(vals):
        """C array of doubles; arrays prepared once per (tableau, step size) are passed through."""
        if isinstance(vals, ctypes.Array):
            return vals
        return (ctypes.c_double * len(vals))(*vals)

    dbl = _dbl

    def rk_stage(self, y, u, Ks, coefs):
        check(self.lib.pn_rk_stage(self.stream(), self.code, self.n, y.data_ptr(), u.data_ptr(),
                                   len(Ks), self._ptrs(Ks), self._dbl(coefs)))

    # the C++ step loops (pn_rk_attempt / pn_rk_adjoint_step) launch this library's HIP entry points themselves
    native_steps = True
    vec_ops = None

    def wrms_buffers(self):
        """(work area, pinned result block) of the error-norm kernel, made on first use."""
        if self.work is None:
            # zero-filled once: the first words are the kernel's arrival counter, which every launch leaves at zero
            self.work = torch.zeros(self.lib.pn_wrms_work_bytes(self.n) // 8 + 1, dtype=torch.float64, device=self.device)
            h, d = ctypes.c_void_p(), ctypes.c_void_p()
            # pinned block the kernel's workgroups store their partial sums into; read_enorm adds them on the host
            check(self.lib.pn_pinned_block(8 * self.lib.pn_wrms_partials(self.n), ctypes.byref(h), ctypes.byref(d)))
            self._err_host, self._err_dev = h, d
        return self.work.data_ptr(), self._err_dev

    def combine_wrms(self, unew, u, Ks, cb, ce, atol, rtol):
        self.wrms_buffers()
        check(self.lib.pn_rk_combine_wrms(self.stream(), self.code, self.n,
                                          None if unew is None else unew.data_ptr(), u.data_ptr(),
                                          len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce),
                                          atol, rtol, self.work.data_ptr(), self._err_dev))

    def read_enorm(self):
        v = ctypes.c_double()
        check(self.lib.pn_stream_wait_wrms(self.stream(), self._err_host, self.n, ctypes.byref(v)))
        return v.value

    # ---- -ts_adapt_wnormtype infinity (pnode_amd/_errnorm.py decides which of the two norms a solve uses)
    infinity_norm = True

    def combine_winf(self, unew, u, Ks, cb, ce, atol, rtol):
        """combine_wrms with the largest term in place of the weighted RMS (pn_rk_combine_winf); read by read_enorm_inf."""
        self.wrms_buffers()
        check(self.lib.pn_rk_combine_winf(self.stream(), self.code, self.n,
                                          None if unew is None else unew.data_ptr(), u.data_ptr(),
                                          len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce),
                                          atol, rtol, self.work.data_ptr(), self._err_dev))

    def read_enorm_inf(self):
        v = ctypes.c_double()
        check(self.lib.pn_stream_wait_winf(self.stream(), self._err_host, self.n, ctypes.byref(v)))
        return v.value

    @property
    def vec_ops_inf(self):
        """pn_vec_ops for the native step loop under the infinity norm: rk_combine_wrms is pn_rk_combine_winf (the same signature),
        the other members stay NULL = this library's entry points."""
        if getattr(self, "_vec_ops_inf", None) is None:
            self._vec_ops_inf_struct = _lib.VecOps()
            self._vec_ops_inf_struct.rk_combine_wrms = ctypes.cast(self.lib.pn_rk_combine_winf, _lib.RK_COMBINE_WRMS_FN)
            self._vec_ops_inf = ctypes.cast(ctypes.pointer(self._vec_ops_inf_struct), ctypes.c_void_p)
        return self._vec_ops_inf

    # ---- per-component tolerances (ODEPetsc.setTolerances; pnode_amd/_errnorm.py decides): vatol, vrtol are fp64 tensors of one
    # period on this device; the norms land in the pinned block and are read by read_enorm / read_enorm_inf
    vector_tolerances = True

    def combine_wrms_v(self, unew, u, Ks, cb, ce, vatol, vrtol):
        """combine_wrms with element e judged against vatol[e % p], vrtol[e % p], p = vatol.numel() (pn_rk_combine_wrms_v)."""
        self.wrms_buffers()
        check(self.lib.pn_rk_combine_wrms_v(self.stream(), self.code, self.n,
                                            None if unew is None else unew.data_ptr(), u.data_ptr(),
                                            len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce),
                                            vatol.data_ptr(), vrtol.data_ptr(), vatol.numel(), self.work.data_ptr(), self._err_dev))

    def combine_winf_v(self, unew, u, Ks, cb, ce, vatol, vrtol):
        """combine_winf with per-component tolerances (pn_rk_combine_winf_v)."""
        self.wrms_buffers()
        check(self.lib.pn_rk_combine_winf_v(self.stream(), self.code, self.n,
                                            None if unew is None else unew.data_ptr(), u.data_ptr(),
                                            len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce),
                                            vatol.data_ptr(), vrtol.data_ptr(), vatol.numel(), self.work.data_ptr(), self._err_dev))

    def adj_theta(self, w, lam, c_lam, dlams, coefs):
        check(self.lib.pn_adj_theta(self.stream(), self.code, self.n, w.data_ptr(),
                                    None if lam is None else lam.data_ptr(), c_lam,
                                    len(dlams), self._ptrs(dlams), self._dbl(coefs)))

    def adj_accum(self, lam_out, lam, dlams, coefs, forcing, w_next=None, c_next=0.0):
        check(self.lib.pn_adj_accum(self.stream(), self.code, self.n, lam_out.data_ptr(), lam.data_ptr(),
                                    len(dlams), self._ptrs(dlams), self._dbl(coefs),
                                    None if forcing is None else forcing.data_ptr(),
                                    None if w_next is None else w_next.data_ptr(), c_next))

    def _segments(self, offsets, lens):
        """ctypes copies of the (constant) parameter layout, built once per layout."""
        key = (id(offsets), id(lens), len(offsets))
        c = self._seg_cache.get(key)
        if c is None:
            n = len(offsets)
            c = ((ctypes.c_int64 * n)(*offsets), (ctypes.c_int64 * n)(*lens), offsets, lens)   # keep the lists alive
            self._seg_cache[key] = c
        return c[0], c[1]

    def param_accum(self, mu, alpha, grads, offsets, lens):
        n = len(grads)
        ptrs = (ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in grads])
        off, ln = self._segments(offsets, lens)
        check(self.lib.pn_param_accum(self.stream(), self.code, mu.data_ptr(), alpha, n, ptrs, off, ln))

    MAX_SOURCES = 32           # gradient sets per pn_param_accum_multi call (include/pnode_amd.h)

    def param_accum_multi(self, mu, alphas, grad_sets, offsets, lens):
        """mu += sum_j alphas[j]*grad_sets[j] (the stages of one or several time steps), added in the
        order j = 0, 1, ...; one call per MAX_SOURCES sets."""
        n = len(offsets)
        off, ln = self._segments(offsets, lens)
        for k in range(0, len(grad_sets), self.MAX_SOURCES):
            sets = grad_sets[k:k + self.MAX_SOURCES]
            ptrs = (ctypes.c_void_p * (n * len(sets)))(*[None if g is None else g.data_ptr() for gs in sets for g in gs])
            check(self.lib.pn_param_accum_multi(self.stream(), self.code, mu.data_ptr(), len(sets),
                                                self._dbl(alphas[k:k + self.MAX_SOURCES]), n, ptrs, off, ln))

    MAX_COLSUM_SOURCES = 32        # sources per pn_colsum_accum_multi call (include/pnode_amd.h)

    def colsum_accum_multi(self, items):
        """For (g, mu, alpha) in items, in order:  mu[c] += alpha * sum_r g[r, c]  (g: rows x cols, contiguous; mu: the slice of
        the flat parameter-sensitivity buffer that belongs to a bias) -- ONE pass over all the g's per <= 32 items."""
        for k in range(0, len(items), self.MAX_COLSUM_SOURCES):
            part = items[k:k + self.MAX_COLSUM_SOURCES]
            n = len(part)
            rows = (ctypes.c_int64 * n)(*[g.shape[0] for g, _, _ in part])
            cols = (ctypes.c_int64 * n)(*[g.shape[1] for g, _, _ in part])
            need = self.lib.pn_colsum_work_bytes(n, rows, cols) // 8 + 1
            w = self._colsum_work
            if w is None or w.numel() < need:
                w = self._colsum_work = torch.empty(need, dtype=torch.float64, device=self.device)
            gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g, _, _ in part])
            mp = (ctypes.c_void_p * n)(*[m.data_ptr() for _, m, _ in part])
            al = (ctypes.c_double * n)(*[a for _, _, a in part])
            check(self.lib.pn_colsum_accum_multi(self.stream(), self.code, n, rows, cols, gp, mp, al, w.data_ptr()))

    def colsum_accum(self, g, mu, alpha):
        self.colsum_accum_multi([(g, mu, alpha)])

    # ---- the fused weight / bias sensitivity kernel of a Linear layer (csrc/pn_linear.hip)
    def linear_wgrad_supported(self, rows, out_f, in_f):
        return bool(self.lib.pn_linear_wgrad_supported(self.code, rows, out_f, in_f))

    def linear_wgrad_buffers(self, out_f, in_f, bias):
        """Zero-filled partial buffers (pw, pb) of one layer: they carry the sum over the stages and steps of a reverse sweep."""
        nb = ctypes.c_int64()
        nw = self.lib.pn_linear_wgrad_work_bytes(self.code, out_f, in_f, ctypes.byref(nb))
        pw = torch.zeros(nw // (4 if self.dtype == torch.float32 else 8), dtype=self.dtype, device=self.device)
        pb = torch.zeros(nb.value // 8, dtype=torch.float64, device=self.device) if bias else None
        return pw, pb

    def linear_wgrad(self, g, x, alpha, pw, pb):
        self.linear_wgrad_group([(g, x, alpha, pw, pb)])

    MAX_WGRAD_PAIRS = _lib.PN_WGRAD_MAX_PAIRS

    wgrad_flags = 0            # PN_WGRAD_EXACT_FP32 with -pn_linear_wgrad_exact 1

    def linear_wgrad_group(self, items, stream=None):
        """The pairs (g, x, alpha, pw, pb) of several layers -- one stage VJP's -- in ONE launch per <= 8 pairs (pn_linear_wgrad_group);
        all g have the same number of rows.  `stream`: a raw stream handle (default: the sweep's stream)."""
        st = self.stream() if stream is None else stream
        for k in range(0, len(items), self.MAX_WGRAD_PAIRS):
            part = items[k:k + self.MAX_WGRAD_PAIRS]
            arr = (_lib.WgradPair * len(part))()
            for q, (g, x, alpha, pw, pb) in zip(arr, part):
                q.g, q.x, q.pw, q.pb = g.data_ptr(), x.data_ptr(), pw.data_ptr(), (None if pb is None else pb.data_ptr())
                q.alpha, q.out_f, q.in_f = alpha, g.shape[1], x.shape[1]
            check(self.lib.pn_linear_wgrad_group(st, self.code, part[0][0].shape[0], len(part), arr, self.wgrad_flags))

    def linear_wgrad_finish(self, out_f, in_f, pw, pb, mu_w, mu_b):
        check(self.lib.pn_linear_wgrad_finish(self.stream(), self.code, out_f, in_f, pw.data_ptr(), None if pb is None else pb.data_ptr(),
                                              mu_w.data_ptr(), None if mu_b is None else mu_b.data_ptr()))

    # ---- the forward of a Linear layer with its activation (pn_linear_fwd, csrc/pn_linear.hip)
    def linear_fwd_supported(self, rows, out_f, in_f):
        return bool(self.lib.pn_linear_fwd_supported(self.code, rows, out_f, in_f))

    linear_flags = 0           # PN_LINEAR_FORM_PLAIN with -pn_linear_form plain: the K loop of linear_fwd / linear_bwd (the same bits)

    linear_relu = True         # linear_fwd and linear_bwd take act="relu" (PN_ACT_RELU; -pn_linear_relu 1)
    linear_sigmoid = True      # ... and act="sigmoid" (PN_ACT_SIGMOID; -pn_linear_sigmoid 1)
    # linear_act_fwd and linear_bwd take act="gelu" (PN_ACT_GELU; -pn_linear_gelu 1), linear_act_fwd a second output z (pn_linear_fwd_pre).
    # linear_fwd keeps refusing the name: its callers save the pair's OUTPUT, and GELU's backward needs the pre-activation
    linear_gelu = True
    linear_softplus = True     # linear_fwd, linear_act_fwd and linear_bwd take act="softplus" (PN_ACT_SOFTPLUS; -pn_linear_softplus 1)
    linear_elu = True          # ... and act="elu" (PN_ACT_ELU; -pn_linear_elu 1)
    _ACTS = {"identity": _lib.PN_ACT_IDENTITY, "tanh": _lib.PN_ACT_TANH, "relu": _lib.PN_ACT_RELU, "sigmoid": _lib.PN_ACT_SIGMOID,
             "softplus": _lib.PN_ACT_SOFTPLUS, "elu": _lib.PN_ACT_ELU}
    _ACTS_PRE = dict(_ACTS, gelu=_lib.PN_ACT_GELU)

    def linear_fwd(self, x, w, b, tanh, y=None, flags=None, act=None):
        """y = act(x w^T + b), act = tanh or the identity; x (rows, in_f), w (out_f, in_f), b (out_f,) or None: contiguous fp32 on this device.
        Refused (PnError), never run another way, outside pn_linear_fwd_supported and where y shares memory with x, w or b.  flags: pn_linear_fwd_form's (default: linear_flags).
        act: None -- `tanh` says which of the two --, or "identity", "tanh", "relu", "sigmoid" by name (`tanh` is then not looked at);
        "relu" gives relu of what the identity gives, value for value; "sigmoid" 1 / (1 + expf(-z)) of it, within 2.5 * 2^-24 of sigma.
        "softplus": nn.Softplus at beta 1, threshold 20 of it (z > 20 ? z : log1pf(expf(z))); "elu": nn.ELU at alpha 1 (z > 0 ? z :
        expm1f(z)).  ("gelu" is linear_act_fwd's.)"""
        if act is not None and act not in self._ACTS:
            raise PnError("pn_linear_fwd: act %r: identity, tanh or relu or sigmoid or softplus or elu (gelu, and the pre-activation beside y: linear_act_fwd)" % (act,))
        return self._linear_fwd(self._ACTS[act] if act is not None else (_lib.PN_ACT_TANH if tanh else _lib.PN_ACT_IDENTITY), x, w, b, y, None, flags)

    def linear_act_fwd(self, x, w, b, act, y=None, z=None, flags=None):
        """linear_fwd with the activation by name only, "gelu" among the names (PN_ACT_GELU: the exact GELU of what the identity gives,
        0.5 z (1 + erff(z / sqrt 2))), and a second output.  z: None -- y alone, pn_linear_fwd_form --, or a (rows, out_f) tensor that
        receives the pre-activation x w^T + b beside y (pn_linear_fwd_pre; any act): the bits of what "identity" gives, and y the bits
        it has without z.  Returns y."""
        if act not in self._ACTS_PRE:
            raise PnError("pn_linear_fwd_pre: act %r: identity, tanh or relu or sigmoid or gelu or softplus or elu" % (act,))
        return self._linear_fwd(self._ACTS_PRE[act], x, w, b, y, z, flags)

    def _linear_fwd(self, code, x, w, b, y, z, flags):
        rows, in_f = x.shape
        out_f = w.shape[0]
        for v in (x, w, b, y, z):
            if v is not None and not (v.is_contiguous() and v.dtype == torch.float32 and v.device == x.device and x.is_cuda):
                raise PnError("pn_linear_fwd: contiguous fp32 tensors on one HIP device")
        if w.shape[1] != in_f or (b is not None and b.numel() != out_f):
            raise PnError("pn_linear_fwd: x (rows, in_f), w (out_f, in_f), b (out_f,)")
        if y is None:
            y = torch.empty((rows, out_f), dtype=x.dtype, device=x.device)
        elif tuple(y.shape) != (rows, out_f):
            raise PnError("pn_linear_fwd: y (rows, out_f)")
        if z is not None:
            if tuple(z.shape) != (rows, out_f):
                raise PnError("pn_linear_fwd: z (rows, out_f)")
            check(self.lib.pn_linear_fwd_pre(self.stream(), _lib.dtype_code(x.dtype), rows, out_f, in_f, x.data_ptr(), w.data_ptr(),
                                             None if b is None else b.data_ptr(), code, y.data_ptr(), z.data_ptr(),
                                             self.linear_flags if flags is None else flags))
            return y
        check(self.lib.pn_linear_fwd_form(self.stream(), _lib.dtype_code(x.dtype), rows, out_f, in_f, x.data_ptr(), w.data_ptr(),
                                          None if b is None else b.data_ptr(), code, y.data_ptr(),
                                          self.linear_flags if flags is None else flags))
        return y

    # ---- the backward of a Linear -> Tanh pair with respect to its input (pn_linear_bwd, csrc/pn_linear.hip)
    def linear_bwd_supported(self, rows, out_f, in_f):
        return bool(self.lib.pn_linear_bwd_supported(self.code, rows, out_f, in_f))

    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        """(gz, dx) = (g (1 - a^2), gz w); g, a (rows, out_f), w (out_f, in_f): contiguous fp32 on this device.  Refused (PnError), never
        run another way, outside pn_linear_bwd_supported, for an fp64 state, and where gz or dx shares memory with an input.
        flags: pn_linear_bwd_form's (default: linear_flags).  act="relu" (pn_linear_bwd_act): gz = threshold_backward(g, a, 0) bit for bit,
        dx the bits of linear_dx(gz, w).  act="sigmoid" (pn_linear_bwd_act): gz = g fmaf(-a, a, a), two roundings, the same bits in every
        form; dx the bits of linear_dx(gz, w).  act="gelu" (pn_linear_bwd_act): `a` is the pair's PRE-activation z; gz = g (cdf + z pdf),
        aten.gelu_backward's formula, the same bits in every form; dx the bits of linear_dx(gz, w).  act="softplus" (pn_linear_bwd_act),
        a the pair's output: gz = g (-expm1f(-a)); act="elu": gz = a > 0 ? g : g (a + 1); the same bits in every form, dx the bits of
        linear_dx(gz, w)."""
        if act not in ("tanh", "relu", "sigmoid", "gelu", "softplus", "elu"):
            raise PnError("pn_linear_bwd: act %r: tanh or relu or sigmoid or gelu or softplus or elu (no activation: linear_dx)" % (act,))
        rows, out_f = g.shape
        in_f = w.shape[1]
        for v in (g, a, w, gz, dx):
            if v is not None and not (v.is_contiguous() and v.dtype == torch.float32 and v.device == g.device and g.is_cuda):
                raise PnError("pn_linear_bwd: contiguous fp32 tensors on one HIP device")
        if tuple(a.shape) != (rows, out_f) or w.shape[0] != out_f:
            raise PnError("pn_linear_bwd: g and a (rows, out_f), w (out_f, in_f)")
        if gz is None:
            gz = torch.empty((rows, out_f), dtype=g.dtype, device=g.device)
        elif tuple(gz.shape) != (rows, out_f):
            raise PnError("pn_linear_bwd: gz (rows, out_f)")
        if dx is None:
            dx = torch.empty((rows, in_f), dtype=g.dtype, device=g.device)
        elif tuple(dx.shape) != (rows, in_f):
            raise PnError("pn_linear_bwd: dx (rows, in_f)")
        flags = self.linear_flags if flags is None else flags
        if act != "tanh":
            check(self.lib.pn_linear_bwd_act(self.stream(), self.code, rows, out_f, in_f, g.data_ptr(), a.data_ptr(), w.data_ptr(), self._ACTS_PRE[act],
                                             gz.data_ptr(), dx.data_ptr(), flags))
        else:
            check(self.lib.pn_linear_bwd_form(self.stream(), self.code, rows, out_f, in_f, g.data_ptr(), a.data_ptr(), w.data_ptr(), gz.data_ptr(),
                                              dx.data_ptr(), flags))
        return gz, dx

    # ---- the backward of a bare Linear layer with respect to its input (pn_linear_dx, csrc/pn_linear.hip)
    def linear_dx_supported(self, rows, out_f, in_f):
        return bool(self.lib.pn_linear_dx_supported(self.code, rows, out_f, in_f))

    def linear_dx(self, g, w, dx=None, flags=None):
        """dx = g w; g (rows, out_f), w (out_f, in_f): contiguous fp32 on this device.  The bits of linear_bwd(g, zeros, w)[1].  Refused
        (PnError), never run another way, outside pn_linear_dx_supported, for an fp64 state, and where dx shares memory with g or w.
        flags: pn_linear_dx_form's (default: linear_flags)."""
        rows, out_f = g.shape
        in_f = w.shape[1]
        for v in (g, w, dx):
            if v is not None and not (v.is_contiguous() and v.dtype == torch.float32 and v.device == g.device and g.is_cuda):
                raise PnError("pn_linear_dx: contiguous fp32 tensors on one HIP device")
        if w.shape[0] != out_f:
            raise PnError("pn_linear_dx: g (rows, out_f), w (out_f, in_f)")
        if dx is None:
            dx = torch.empty((rows, in_f), dtype=g.dtype, device=g.device)
        elif tuple(dx.shape) != (rows, in_f):
            raise PnError("pn_linear_dx: dx (rows, in_f)")
        check(self.lib.pn_linear_dx_form(self.stream(), self.code, rows, out_f, in_f, g.data_ptr(), w.data_ptr(), dx.data_ptr(),
                                         self.linear_flags if flags is None else flags))
        return dx

    # ---- dense output (-pn_output_times interpolate; csrc/pn_dense.hip)
    dense_flags = _lib.PN_DENSE_NONTEMPORAL      # output rows are not read again by the sweep: non-temporal stores

    def dense_eval(self, out, u, Ks, coefs):
        """out[o] = u + sum_j coefs[o][j]*Ks[j] for every row o of the 2-D view `out` (rows of the solution tensor): ONE launch
        per PN_DENSE_CHUNK rows (pn_rk_dense_eval)."""
        m, nk = len(coefs), len(Ks)
        c = (ctypes.c_double * (m * nk))(*[x for row in coefs for x in row])
        check(self.lib.pn_rk_dense_eval(self.stream(), self.code, self.n, u.data_ptr(), nk, (ctypes.c_void_p * nk)(*[k.data_ptr() for k in Ks]),
                                        m, c, out.data_ptr(), out.stride(0), self.dense_flags))

    def dense_adjoint(self, Ds, G, g, coefs, accumulate=False):
        """Ds[j] (+)= sum_o coefs[o][j]*g[o], G (+)= sum_o g[o] (G may be None) over the rows of the 2-D view `g`, o ascending
        (pn_rk_dense_adjoint)."""
        m, nd = g.shape[0], len(Ds)
        c = (ctypes.c_double * max(m * nd, 1))(*[x for row in coefs for x in row])
        check(self.lib.pn_rk_dense_adjoint(self.stream(), self.code, self.n, m, g.data_ptr(), g.stride(0), nd, c,
                                           (ctypes.c_void_p * max(nd, 1))(*[d.data_ptr() for d in Ds]),
                                           None if G is None else G.data_ptr(), 1 if accumulate else 0))

    def _tgrad_work(self):
        w = getattr(self, "_tg_work", None)
        if w is None:                               # arrival counters start at zero (pn_tgrad_work_bytes)
            w = self._tg_work = torch.zeros(self.lib.pn_tgrad_work_bytes(self.n) // 8, dtype=torch.float64, device=self.device)
        return w

    def tgrad_dots(self, acc, xs, ys, coefs, accumulate=True):
        """acc[0] (+)= sum_p coefs[p] * <xs[p], ys[p]> in double, fixed order (pn_tgrad_dots); `acc`: a slot of an fp64 tensor."""
        np_ = len(xs)
        check(self.lib.pn_tgrad_dots(self.stream(), self.code, self.n, np_, (ctypes.c_void_p * np_)(*[x.data_ptr() for x in xs]),
                                     (ctypes.c_void_p * np_)(*[y.data_ptr() for y in ys]), (ctypes.c_double * np_)(*coefs),
                                     self._tgrad_work().data_ptr(), acc.data_ptr(), 1 if accumulate else 0))

    def dense_tgrad(self, acc, g, Ks, coefs, accumulate=True):
        """acc[o] (+)= sum_j coefs[o][j] * <g[o], Ks[j]> for the rows o of the 2-D view `g` (pn_rk_dense_tgrad)."""
        m, nk = g.shape[0], len(Ks)
        c = (ctypes.c_double * (m * nk))(*[x for row in coefs for x in row])
        check(self.lib.pn_rk_dense_tgrad(self.stream(), self.code, self.n, m, g.data_ptr(), g.stride(0), nk,
                                         (ctypes.c_void_p * nk)(*[k.data_ptr() for k in Ks]), c, self._tgrad_work().data_ptr(),
                                         acc.data_ptr(), 1 if accumulate else 0))

    # ---- per-sample step control (-pn_adapt_scope sample; csrc/pn_rows.hip): the state is B rows of d entries
    def f64(self, *shape):
        return torch.zeros(*shape, dtype=torch.float64, device=self.device)

    def i32(self, *shape):
        return torch.zeros(*shape, dtype=torch.int32, device=self.device)

    def rows_stage(self, B, d, y, u, Ks, coefs, h):
        check(self.lib.pn_rows_stage(self.stream(), self.code, B, d, y.data_ptr(), u.data_ptr(), len(Ks), self._ptrs(Ks),
                                     self._dbl(coefs), h.data_ptr()))

    def rows_combine_wrms(self, B, d, unew, u, Ks, cb, ce, h, atol, rtol, enorm):
        check(self.lib.pn_rows_combine_wrms(self.stream(), self.code, B, d, None if unew is None else unew.data_ptr(), u.data_ptr(),
                                            len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce), h.data_ptr(), atol, rtol,
                                            enorm.data_ptr()))

    def rows_combine_winf(self, B, d, unew, u, Ks, cb, ce, h, atol, rtol, enorm):
        """rows_combine_wrms with every row's largest term in `enorm` (pn_rows_combine_winf)."""
        check(self.lib.pn_rows_combine_winf(self.stream(), self.code, B, d, None if unew is None else unew.data_ptr(), u.data_ptr(),
                                            len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce), h.data_ptr(), atol, rtol,
                                            enorm.data_ptr()))

    def rows_combine_wrms_v(self, B, d, unew, u, Ks, cb, ce, h, vatol, vrtol, enorm):
        """rows_combine_wrms with column c judged against vatol[c], vrtol[c]: d entries each (pn_rows_combine_wrms_v)."""
        check(self.lib.pn_rows_combine_wrms_v(self.stream(), self.code, B, d, None if unew is None else unew.data_ptr(), u.data_ptr(),
                                              len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce), h.data_ptr(), vatol.data_ptr(),
                                              vrtol.data_ptr(), vatol.numel(), enorm.data_ptr()))

    def rows_combine_winf_v(self, B, d, unew, u, Ks, cb, ce, h, vatol, vrtol, enorm):
        """rows_combine_winf with per-column tolerances (pn_rows_combine_winf_v)."""
        check(self.lib.pn_rows_combine_winf_v(self.stream(), self.code, B, d, None if unew is None else unew.data_ptr(), u.data_ptr(),
                                              len(Ks), self._ptrs(Ks), self._dbl(cb), self._dbl(ce), h.data_ptr(), vatol.data_ptr(),
                                              vrtol.data_ptr(), vatol.numel(), enorm.data_ptr()))

    def rows_control(self, ts, B, nspan, span, max_time, enorm, sd, si, log_d, log_hit, accept, summary):
        """One judgement per unfinished row (pn_rows_control); `summary` is read by rows_summary."""
        w = getattr(self, "_rows_work", None)
        if w is None or w.numel() * 8 < self.lib.pn_rows_work_bytes(B):        # arrival counters start at zero
            w = self._rows_work = torch.zeros(self.lib.pn_rows_work_bytes(B) // 8, dtype=torch.float64, device=self.device)
        check(self.lib.pn_rows_control(self.stream(), ts, B, nspan, None if span is None else span.data_ptr(), max_time,
                                       enorm.data_ptr(), sd.data_ptr(), si.data_ptr(), log_d.data_ptr(), log_hit.data_ptr(),
                                       accept.data_ptr(), summary.data_ptr(), w.data_ptr()))

    def rows_summary(self, summary):
        """(rows still unfinished, first failing row or -1, its failure code): the one read-back of a round."""
        v = summary.tolist()
        return v[0], v[1], v[2]

    def rows_commit(self, B, d, unext, u, unew, accept, hit, sol, ld, nout):
        check(self.lib.pn_rows_commit(self.stream(), self.code, B, d, unext.data_ptr(), u.data_ptr(), unew.data_ptr(),
                                      accept.data_ptr(), None if hit is None else hit.data_ptr(),
                                      None if sol is None else sol.data_ptr(), ld, nout))

    def rows_adj_theta(self, B, d, w, lam, c_lam, dlams, coefs, h, dense_w=None):
        """`dense_w`: the D_i of the rows' interpolated outputs, added last and not scaled by h (pn_rows_adj_theta_dense)."""
        if dense_w is not None:
            check(self.lib.pn_rows_adj_theta_dense(self.stream(), self.code, B, d, w.data_ptr(), None if lam is None else lam.data_ptr(),
                                                   c_lam, len(dlams), self._ptrs(dlams), self._dbl(coefs), h.data_ptr(),
                                                   dense_w.data_ptr()))
            return
        check(self.lib.pn_rows_adj_theta(self.stream(), self.code, B, d, w.data_ptr(), None if lam is None else lam.data_ptr(),
                                         c_lam, len(dlams), self._ptrs(dlams), self._dbl(coefs), h.data_ptr()))

    # ... with -pn_output_times interpolate: the rows serve the output times themselves
    rows_dense = True

    def rows_dense_eval(self, B, d, sol, times, u, Ks, P, unew, log_d, tnew, log_hit, nxt, rng):
        """The outputs of a round (pn_rows_dense_eval): `sol` the 2-D view of the solution tensor, `times` its output times on the
        device, `P` the used rows of the extension's table (a C array of len(Ks) * PN_DENSE_MAX_POW doubles)."""
        check(self.lib.pn_rows_dense_eval(self.stream(), self.code, B, d, u.data_ptr(), len(Ks), self._ptrs(Ks), P, unew.data_ptr(),
                                          sol.data_ptr(), sol.stride(0), sol.shape[0], times.data_ptr(), log_d.data_ptr(),
                                          tnew.data_ptr(), log_hit.data_ptr(), nxt.data_ptr(), rng.data_ptr()))

    def rows_dense_adjoint(self, B, d, Ds, G, g, times, P, rng, log_d):
        """Ds[j][r] = sum_o c_ojr g[o][r], G[r] = sum_o g[o][r] over the row's logged range (pn_rows_dense_adjoint)."""
        check(self.lib.pn_rows_dense_adjoint(self.stream(), self.code, B, d, g.data_ptr(), g.stride(0), g.shape[0], times.data_ptr(),
                                             log_d.data_ptr(), rng.data_ptr(), len(Ds), P, self._ptrs(Ds), G.data_ptr()))

    # ... and dL/dt of such a solve: row-wise reductions, the per-row scatter, one ordered sum over rows
    rows_tgrad = True

    def rows_tgrad_dots(self, B, d, rowacc, xs, ys, coefs, accumulate=True):
        """rowacc[r] (+)= sum_p coefs[p] * <xs[p][r], ys[p][r]> in double (pn_rows_tgrad_dots)."""
        np_ = len(xs)                                      # (two pointer tables in one call: _ptrs' one array serves the first)
        check(self.lib.pn_rows_tgrad_dots(self.stream(), self.code, B, d, np_, self._ptrs(xs),
                                          (ctypes.c_void_p * np_)(*[y.data_ptr() for y in ys]), self._dbl(coefs),
                                          rowacc.data_ptr(), 1 if accumulate else 0))

    def rows_dense_tgrad(self, B, d, erow, g, Ks, times, P, rng, log_d):
        """erow[o][r] = sum_j beta'_j(theta_or) <g[o][r], Ks[j][r]> over the row's logged range (pn_rows_dense_tgrad)."""
        check(self.lib.pn_rows_dense_tgrad(self.stream(), self.code, B, d, g.data_ptr(), g.stride(0), g.shape[0], times.data_ptr(),
                                           log_d.data_ptr(), rng.data_ptr(), len(Ks), P, self._ptrs(Ks), erow.data_ptr()))

    def _tgrad_scatter_args(self, B, dtrow, rowacc, tbars, coefs, tbar0, c_last, fsal, log_d, hit, rng, erow, times, held, iv, flush):
        opt = lambda x: None if x is None else x.data_ptr()
        return (B, dtrow.shape[0], dtrow.data_ptr(), opt(rowacc), len(tbars), self._ptrs(tbars) if tbars else None,
                self._dbl(coefs) if tbars else None, opt(tbar0), c_last, 1 if fsal else 0, opt(log_d), opt(hit), opt(rng), opt(erow),
                opt(times), held.data_ptr(), iv.data_ptr(), 1 if flush else 0)

    def rows_tgrad_scatter(self, B, dtrow, rowacc, tbars, coefs, tbar0, c_last, fsal, log_d, hit, rng, erow, times, held, iv, flush=False):
        """One reversed round (or, with `flush`, what the rows still hold after the last one) into every row's own column of the
        fp64 matrix `dtrow` [T][B] (pn_rows_tgrad_scatter); `tbars`: fp64 vectors of B entries, <w_j, df/dt> per row."""
        check(self.lib.pn_rows_tgrad_scatter(self.stream(), *self._tgrad_scatter_args(B, dtrow, rowacc, tbars, coefs, tbar0, c_last, fsal,
                                                                                      log_d, hit, rng, erow, times, held, iv, flush)))

    def rows_tgrad_reduce(self, B, dtrow, dt):
        """dt[i] = sum_r dtrow[i][r] in a fixed order (pn_rows_tgrad_reduce)."""
        T = dtrow.shape[0]
        need = self.lib.pn_rows_tgrad_work_bytes(B, T)
        w = getattr(self, "_rows_tg_work", None)
        if w is None or w.numel() * 8 < need:             # arrival counters start at zero
            w = self._rows_tg_work = torch.zeros(need // 8, dtype=torch.float64, device=self.device)
        check(self.lib.pn_rows_tgrad_reduce(self.stream(), B, T, dtrow.data_ptr(), dt.data_ptr(), w.data_ptr()))

    # ... and -pn_rows_compact 1: func sees the rows of a round that have work to do
    rows_compact = True

    def rows_list(self, B, kind, src, idx, pos, count):
        """The ordered list of the rows with work to do (pn_rows_list): kind 0, `src` the int32 `finished` row of si (listed: 0);
        kind 1, `src` the fp64 h_eff row of a round's log (listed: > 0).  idx, pos: int32 [B]; count: int32, one entry."""
        check(self.lib.pn_rows_list(self.stream(), B, kind, src.data_ptr(), idx.data_ptr(), pos.data_ptr(), count.data_ptr(), None))

    def rows_gather(self, m, d, out, src, idx):
        """out[k] = src[idx[k]] for k < m, rows of d entries of out's dtype (pn_rows_gather)."""
        check(self.lib.pn_rows_gather(self.stream(), _lib.dtype_code(out.dtype), m, d, out.data_ptr(), src.data_ptr(), idx.data_ptr()))

    def rows_scatter(self, B, d, out, src, pos):
        """out[r] = src[pos[r]] where pos[r] >= 0, else +0, for every r < B (pn_rows_scatter)."""
        check(self.lib.pn_rows_scatter(self.stream(), _lib.dtype_code(out.dtype), B, d, out.data_ptr(),
                                       src.data_ptr() if src.numel() else None, pos.data_ptr()))

    def rows_adj_accum(self, B, d, lam_out, lam, dlams, g, ld, hit, nout):
        check(self.lib.pn_rows_adj_accum(self.stream(), self.code, B, d, lam_out.data_ptr(), lam.data_ptr(), len(dlams),
                                         self._ptrs(dlams), None if g is None else g.data_ptr(), ld,
                                         None if hit is None else hit.data_ptr(), nout))

    def copy(self, y, x):
        check(self.lib.pn_copy(self.stream(), self.code, self.n, y.data_ptr(), x.data_ptr()))

    def lincomb(self, out, xs, cs):
        check(self.lib.pn_lincomb(self.stream(), self.code, self.n, out.data_ptr(), len(xs), self._ptrs(xs), self._dbl(cs)))

    def dots(self, x, ys):
        """[<x, y_j>] as Python floats; any number of vectors, ONE host synchronisation."""
        nmax = 64
        if self.dots_work is None:
            per = (self.lib.pn_dots_work_bytes(self.n) // 8 + 2) // 2 * 2          # every chunk's area stays 16-byte aligned
            self._dots_per = per
            self.dots_work = torch.zeros(per * (nmax // 8), dtype=torch.float64, device=self.device)   # arrival counters start at zero
            h, d = ctypes.c_void_p(), ctypes.c_void_p()
            check(self.lib.pn_pinned_block(8 * nmax, ctypes.byref(h), ctypes.byref(d)))
            self._dots_host, self._dots_dev = h, d
        if len(ys) > nmax:
            return self.dots(x, ys[:nmax]) + self.dots(x, ys[nmax:])
        st = self.stream()
        for c, k in enumerate(range(0, len(ys), 8)):
            chunk = ys[k:k + 8]
            check(self.lib.pn_dots(st, self.code, self.n, x.data_ptr(), len(chunk), self._ptrs(chunk),
                                   self.dots_work.data_ptr() + 8 * c * self._dots_per,
                                   ctypes.c_void_p(self._dots_dev.value + 8 * k)))
        vals = (ctypes.c_double * len(ys))()
        check(self.lib.pn_stream_wait_scalars(st, self._dots_host, len(ys), vals))
        return list(vals)

    # ---- device-resident GMRES (include/pnode_amd.h section 3c).  `reduce`: None, or a callable that sums a small
    # device tensor over the ranks in stream order (the products must be global before GMRES decides anything)
    MAX_KRYLOV_RESTART = 126

    def krylov_new(self, restart):
        return _KrylovBuffers(self, restart)

    def krylov_begin(self, kr, r, rtol, atol, maxit, first, reduce=None):
        st, lib = self.stream(), self.lib
        args = (st, self.code, self.n, kr.m, kr.state.data_ptr(), kr.status_dev, r.data_ptr(), kr.V.data_ptr(), kr.npad,
                kr.vin.data_ptr(), rtol, atol, int(min(maxit, 2 ** 62)), 1 if first else 0)
        if reduce is None:
            check(lib.pn_krylov_begin(*(args + (0,))))
        else:
            check(lib.pn_krylov_begin(*(args + (1,))))
            reduce(kr.products(1))
            check(lib.pn_krylov_begin(*(args + (2,))))

    def krylov_step(self, kr, k, reduce=None):
        st, lib = self.stream(), self.lib
        args = (st, self.code, self.n, kr.m, kr.state.data_ptr(), kr.status_dev, k, kr.w.data_ptr(), kr.V.data_ptr(), kr.npad,
                kr.vin.data_ptr())
        if reduce is None:
            check(lib.pn_krylov_step(*(args + (0,))))
        else:
            check(lib.pn_krylov_step(*(args + (1,))))
            reduce(kr.products(k + 2))
            check(lib.pn_krylov_step(*(args + (2,))))
            reduce(kr.products(k + 2))
            check(lib.pn_krylov_step(*(args + (3,))))

    def krylov_close(self, kr, x):
        check(self.lib.pn_krylov_close(self.stream(), self.code, self.n, kr.m, kr.state.data_ptr(), kr.status_dev,
                                       x.data_ptr(), kr.V.data_ptr(), kr.npad))

    def krylov_status(self, kr):
        """(stop, iterations of this cycle, iterations of the solve, residual-norm estimate) -- waits for the stream."""
        v = kr._vals
        check(self.lib.pn_stream_wait_scalars(self.stream(), kr.status_host, 8, v))
        kr.second_passes = int(v[7])                     # of this solve so far (diagnostic)
        return int(v[0]), int(v[1]), int(v[2]), v[3]


class _KrylovBuffers(object):
    """Device memory of one GMRES solver (pn_krylov_*, include/pnode_amd.h section 3c): the Krylov vectors, the
    operator's input and output buffers, the state block GMRES keeps its decisions in and the pinned status block."""

    def __init__(self, ops, restart):
        lib = ops.lib
        self.m = restart
        self.npad = (ops.n + 63) // 64 * 64
        self.V = ops.empty(restart + 1, self.npad)
        self.vin = ops.empty(self.npad)
        self.w = ops.empty(self.npad)
        nd = lib.pn_krylov_state_doubles(ops.n, restart)
        if nd <= 0:
            raise PnError("pn_krylov: restart length %d is outside 1..126" % restart)
        self.state = torch.zeros(nd, dtype=torch.float64, device=ops.device)      # arrival counter starts at zero
        self.hoff = lib.pn_krylov_products_offset(restart)
        h, d = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib.pn_pinned_block(64, ctypes.byref(h), ctypes.byref(d)))
        self.status_host, self.status_dev = h, d
        self._lib = lib
        self._vals = (ctypes.c_double * 8)()

    def __del__(self):
        try:
            if self.status_host.value:
                self._lib.pn_pinned_free(self.status_host)
        except Exception:
            pass

    def products(self, count):
        """The Gram-Schmidt products of the pass in flight (for the sum over the ranks)."""
        return self.state[self.hoff: self.hoff + count]
