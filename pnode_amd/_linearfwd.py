"""func's ``nn.Linear`` layers, alone or with the activation behind them, as ONE launch in the solver's own evaluations of func
(``pn_linear_fwd`` and its siblings, csrc/pn_linear.hip).

The body of ``evalRHSFunction`` (pa.py:393-412) at BASELINE's target configuration is four library GEMMs and three elementwise
``tanh`` launches; each ``tanh`` moves 16 MiB in about 6 us, twice what its traffic needs -- mostly dispatch floor.  A Linear and the
activation behind it are therefore run as one MFMA kernel with the bias and the activation in its epilogue.

THE RULES, the same for every kind of owned layer.  A pair is owned where ALL of this holds:

* the pair is two consecutive children of an ``nn.Sequential`` whose ``forward`` is ``nn.Sequential``'s own; the first is exactly
  ``nn.Linear`` (no subclass; weight and bias trainable parameters of the solver, owned by no other module -- the rules of
  ``LinearParamGrads.install``), the second exactly the kind's module class with the parameters the kernel has (``_static_why`` and the
  kind's ``param_why``; the activation module itself is never called, so either ``inplace`` will do);
* neither module nor the container carries a hook that is not the engine's own, and no global module hook is registered;
* at call time (``_fusable``): the input is a contiguous CUDA fp32 tensor of the state's dtype, autocast is off,
  ``pn_linear_fwd_supported``.

Anything else runs the stock modules.  Only evaluations inside ``LinearFwd.window`` are affected -- the solver opens it around its own
calls of func; for its duration the eligible containers carry an instance-level ``forward`` (the runner below), removed when the window
closes, also when func raises: func is left exactly as found (pnode_amd/_funcguard.py sees no change between two calls).

Autograd: a pair is one ``torch.autograd.Function`` (``_LinearTanh``, for every kind) that saves ``(x, w, s)``, ``s`` the tensor the
activation's derivative is a function of.  Its backward forms ``g_z = g act'(s)`` and ``dx = g_z W`` in ONE launch (the prologue in
registers, W read as it lies) where the backend has the entry and the kind's capability flag, ``-pn_linear_bwd`` is not ``0``, the input
needs a gradient, ``g`` is a contiguous, 16-byte aligned fp32 tensor of the pair's shape on the weight's device, autocast is off, the
backward is not itself differentiated and ``pn_linear_bwd_supported`` (``_bwd_fusable``); otherwise with the torch operations autograd
runs for the stock modules (the kind's ``gz``, then ``matmul``).  Either way the backward hands ``(g_z, x)`` to
``LinearParamGrads._grad_hook`` (the queue, the grouped launch, the side stream, the deferral under per-evaluation graphs) when that is
active for the evaluation; otherwise it returns ``dW = g_z^T x`` and ``db = colsum(g_z)`` to autograd.  ``Evaluation.clean`` sees the
pair's node as it sees a hooked layer: the walk goes on along the input edge only.

Self-checks, per kind and per solver.  The first fused call of a kind outside a capture is computed through torch as well, and so is
its first fused backward: ``dx`` must agree to 1e-6 of ``|g_z| |W|``, the forward and ``g_z`` to the kind's bars below.  A check that
finds no cell to judge by leaves the next call to be checked.  A miss switches off that kind's forward (``why``), or that kind's
backward (``bwd_why``; its forward stays), and nothing else; the call returns the torch results.  Under stream capture nothing is
checked.  Each record counts the calls that ran as one launch (``n``, ``n_bwd``): a call only after it passed or skipped its check.

THE TABLE.  ``KINDS`` has one ``_Kind`` per kind of owned layer -- tanh, relu, sigmoid, gelu, softplus, elu, bare -- and holds everything
that differs between them; no code outside it asks which kind it has.  Its columns:

``key``            the backend's name of the activation (``act=`` of ``linear_fwd`` / ``linear_bwd``), the stem of the option and of
                   ``LinearFwd``'s names;
``module``, ``param_why``  the module class, and the reason (or None) a module of that class has parameters the kernel has no slot for;
``option``, ``always``  tanh pairs are always looked for and ``-pn_linear_fwd auto|0|1`` governs them (as it does every kind: with ``0``
                   there is no ``LinearFwd``); every other kind only with its own ``-pn_linear_<key> 1`` (default ``0``: nothing happens);
``class_key``      ``find_layers`` reports a pair that cannot be owned under the container's class name alone (tanh) or under
                   ``(class name, name)``;
``call_fwd``, ``call_bwd``  the form of the call into the backend (``_fwd_tanh`` ... ``_bwd_bare``); ``capability`` the flag of the backend
                   the backward needs beside ``bwd_entry`` (``linear_<key>``; none where not ``flagged``); ``bwd_kernel`` the kernel's name in the messages;
``saves_pre``      the derivative is a function of the PRE-activation (GELU), not of the output;
``fwd``, ``torch_fwd``, ``gz``, ``gz_text``  the torch expressions the pair replaces, and their wording in the messages;
``check``          the form of the forward check: ``_relative`` -- cells with ``sum |x w| + |b| > 0``, the difference at most 1e-6 of it (the
                   library path's own 1.0e-7, the split product's 5.7e-8 and a few ulp of the activation, with room) -- or ``_barred``
                   -- cells with a finite scale, the bar ``1e-6 (sum |x w| + |b|) + 4 * 2^-24`` for the activations that do not map a
                   zero pre-activation to an exact 0;
``gz_bar``         the bar of ``g_z`` in units of ``2^-24 |g|``, or None: bit for bit;
``says``           what the status adds to its text; ``legacy`` the names ``LinearFwd`` has for the record's fields.

A ``LinearFwd`` has one ``_PairState`` per row (``records``): the row's fields and, beside them, all that changes while a solver runs
-- the plans, the option's value, the checks' flags and reasons, the counters, the warn-once flags.

THE KINDS, what is particular to each.

Tanh: the first kind and the one with the older entry points -- ``linear_fwd(x, w, b, True)`` and ``linear_bwd(g, a, w)``
(``pn_linear_bwd``) without ``act=``, no capability flag.  ``g_z = g_a (1 - a^2)``.

ReLU: ``g_z`` has no arithmetic in it, so it must be ``threshold_backward``'s bit for bit, and a ``g_z`` that is not is a miss even
where no cell of ``dx`` can be judged.  ReLU is 1-Lipschitz: the bare layer's forward bar carries over.

Sigmoid: ``g_z = g a (1 - a)``.  The first kind with the barred forward check: sigma maps a zero pre-activation to 0.5 with a rounding
of its own on either side (the kernel at most 2.5 ulp of 2^-24, the library about 1), where tanh and ReLU give an exact 0.

GELU (exact only; ``approximate='tanh'`` is refused with its reason): the SAVED PRE-ACTIVATION kind.  GELU is not monotonic: its
derivative needs ``z = x W^T + b``, which cannot be had back from the output.  An evaluation that will be differentiated (grad mode on
and the input or a parameter requires a gradient) launches ``pn_linear_fwd_pre`` -- ``y`` and ``z`` from one epilogue; ``(x, w, z)`` is
saved and ``y`` is not: the memory of the stock pair.  Any other evaluation (the forward sweep without retained tapes) launches
``pn_linear_fwd`` with ``PN_ACT_GELU``, allocates no ``z`` and saves nothing.  Both go through ``linear_act_fwd`` (``linear_fwd`` refuses
the name).  ``n`` counts both, ``n_pre`` the first, ``n_y`` the second.  The forward check also holds ``z``, where the call wrote it,
against ``F.linear`` under the same bar.  Backward: ``g_z = g (cdf + z pdf)``.

Softplus (``beta == 1`` and ``threshold == 20`` only) and ELU (``alpha == 1`` only): both derivatives are functions of the OUTPUT,
``1 - e^-a`` and ``a > 0 ? 1 : a + 1``.  Softplus maps a zero pre-activation to ``log 2``, and ELU's rows of scale 0 are an exact 0 and
need a bar above 0: the barred forward check.

Bare (``-pn_linear_bare 0|1``): a child of an eligible container that is exactly ``nn.Linear``, opens no owned pair and passes the
static rules of a pair's Linear -- the head of every ``... -> Linear`` net, a Linear in front of an activation whose option is off or
of a subclass of ``nn.Tanh``.  It runs through ``_Linear``: forward ``linear_fwd(x, w, b, False)`` under ``_fusable``; backward
``dx = g W`` by ``pn_linear_dx`` (the kernel body of ``pn_linear_bwd`` without the prologue: no ``a`` read, no ``g_z`` written) under the
rules of ``_bwd_fusable`` minus everything about ``a``, else ``matmul``; ``(g, x)`` goes to ``LinearParamGrads._grad_hook`` as a pair's
``(g_z, x)`` does.  A container whose only eligible members are bare layers is active too.  Neither a refused call nor a refused
backward warns."""
import contextlib
import warnings
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

CHECK_TOL = 1e-6


def _global_hooks():
    mod = torch.nn.modules.module
    for name in ("_global_forward_hooks", "_global_forward_pre_hooks", "_global_backward_hooks", "_global_backward_pre_hooks",
                 "_global_forward_hooks_always_called"):
        if getattr(mod, name, None):
            return True
    return False


def _autocast_on(device_type):
    try:
        return bool(torch.is_autocast_enabled(device_type))
    except TypeError:                                  # (an older spelling: the HIP device's state, and the host's)
        return bool(torch.is_autocast_enabled() or (device_type == "cpu" and torch.is_autocast_cpu_enabled()))


def _user_hooked(m):
    """True when `m` carries a forward, pre-forward or backward hook that is not the engine's own (the forward hook of a solver's
    LinearParamGrads -- this solver's or another's on the same func: it acts only while ITS solver records an evaluation)."""
    from ._lineargrad import LinearParamGrads
    for name in ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks"):
        for h in (getattr(m, name, None) or {}).values():
            if not isinstance(getattr(h, "__self__", None), LinearParamGrads):
                return True
    return False


def _static_why(seq, kids, lin, act, index, owners, kind=nn.Tanh):
    """The static half of the eligibility rules for the Linear `lin` (and the activation `act` behind it, exactly a `kind`, the module
    class of a row of KINDS; None for a bare layer) among the children `kids` of `seq`: None, or the reason as a string."""
    mods = (lin,) if act is None else (lin, act)
    if type(seq) is not nn.Sequential or "forward" in seq.__dict__:
        return "the container's forward is not nn.Sequential's own"
    if type(lin) is not nn.Linear or (act is not None and type(act) is not kind):
        return "a subclass of nn.Linear or nn.%s" % kind.__name__
    if any("forward" in m.__dict__ for m in mods):
        return "an instance-level forward on the layer"
    why = None
    for p in (lin.weight, lin.bias):
        if p is None:
            continue
        if not isinstance(p, nn.Parameter) or not p.requires_grad or id(p) not in index:
            why = "a weight or bias that is not a trainable parameter of the solver"
        elif owners.get(id(p), 0) != 1:
            why = "a weight or bias shared with another module"
    if why is None and sum(kids.count(m) for m in mods) != len(mods):
        why = "the layer appears twice in the container"
    return why


# ---- what the rows of KINDS are made of: the parameter rules, the torch expressions, the forms of the backend call and of the check
def _gelu_why(act):
    if getattr(act, "approximate", "none") != "none":
        return "nn.GELU(approximate=%r): only the exact GELU (approximate='none') is owned" % (act.approximate,)
    return None


def _softplus_why(act):
    if act.beta != 1 or act.threshold != 20:
        return "nn.Softplus(beta=%r, threshold=%r): only beta == 1 and threshold == 20 are owned" % (act.beta, act.threshold)
    return None


def _elu_why(act):
    if act.alpha != 1.0:
        return "nn.ELU(alpha=%r): only alpha == 1 is owned" % (act.alpha,)
    return None


def _relu_gz(g, a):
    return torch.ops.aten.threshold_backward(g, a, 0)


def _gelu_gz(g, z):
    return torch.ops.aten.gelu_backward(g, z, approximate="none")


def _softplus_gz(g, a):
    return g * (-torch.expm1(-a))


def _elu_gz(g, a):
    return torch.ops.aten.elu_backward(g, 1, 1, 1, True, a)


def _identity(z):
    return z


# the one place the device is touched.  (ops, key, x2, w, b, z) -> y; z: None, or the tensor the pre-activation goes to
def _fwd_tanh(ops, key, x2, w, b, z):
    return ops.linear_fwd(x2, w, b, True)


def _fwd_bare(ops, key, x2, w, b, z):
    return ops.linear_fwd(x2, w, b, False)


def _fwd_act(ops, key, x2, w, b, z):
    return ops.linear_fwd(x2, w, b, False, act=key)


def _fwd_pre(ops, key, x2, w, b, z):
    return ops.linear_act_fwd(x2, w, b, key) if z is None else ops.linear_act_fwd(x2, w, b, key, z=z)


# (ops, key, g2, s2, w) -> (g_z, dx); a bare layer: dx alone
def _bwd_tanh(ops, key, g2, s2, w):
    return ops.linear_bwd(g2, s2, w)


def _bwd_act(ops, key, g2, s2, w):
    return ops.linear_bwd(g2, s2, w, act=key)


def _bwd_bare(ops, key, g2, s2, w):
    return ops.linear_dx(g2, w)


# the two forms of the forward check.  (kind, a, ref, z, lin, scale) -> (True when there was a cell to judge by, None or the miss)
def _relative(kind, a, ref, z, lin, scale):
    ok = torch.isfinite(ref) & (scale > 0)
    if not bool(ok.any()):
        return False, None
    err = float(((a - ref).abs() / scale)[ok].max())
    if err <= CHECK_TOL:
        return True, None
    return True, "pn_linear_fwd and %s differ by %.2e of sum |x w| + |b| (allowed: %.0e)" % (kind.torch_fwd, err, CHECK_TOL)


def _barred(kind, a, ref, z, lin, scale):
    ok = torch.isfinite(ref) & torch.isfinite(scale)
    if not bool(ok.any()):
        return False, None
    bar = CHECK_TOL * scale + 4.0 * 2.0 ** -24
    over = ((a - ref).abs() / bar)[ok].max()
    what = "pn_linear_fwd and %s" % kind.torch_fwd
    if z is not None and float(over) <= 1.0:      # the pre-activation, where the call wrote it: against F.linear under the same bar
        over = ((z.reshape(ref.shape) - lin).abs() / bar)[ok].max()
        what = "the pre-activation of pn_linear_fwd_pre and F.linear"
    if float(over) <= 1.0:
        return True, None
    return True, "%s differ by %.2f times the bar %.0e (sum |x w| + |b|) + 4 * 2^-24" % (what, float(over), CHECK_TOL)


_FLAGS = ("mode", "disabled", "why", "checked", "bwd_disabled", "bwd_why", "bwd_checked")


def _legacy(stem, fields, plans=None, record=None, count=None):
    """{name on LinearFwd: field of the record, None for the record itself}: `fields` under `stem`_<field>, the two counters under
    n_<count or stem> and n_<count or stem>_bwd, the plans and the record under the names given."""
    names = {(stem + "_" + f if stem else f): f for f in fields}
    names.update({"n_" + (count or stem): "n", "n_%s_bwd" % (count or stem): "n_bwd"})
    if plans is not None:
        names[plans] = "plans"
    if record is not None:
        names[record] = None
    return names


class _Kind(object):
    """One row of KINDS (the columns: the module's docstring).  What is not given is what a kind added as a PN_ACT_* code has."""
    def __init__(self, key, module, torch_fwd, fwd, gz_text, gz, gz_bar, check, legacy, param_why=None, option=None, always=False,
                 class_key=False, call_fwd=_fwd_act, call_bwd=_bwd_act, flagged=True, bwd_entry="linear_bwd",
                 bwd_kernel="pn_linear_bwd_act", saves_pre=False, says=(), none=None, plural="pairs", fwd_off=None):
        self.key, self.module, self.param_why = key, module, param_why
        self.name = module.__name__
        self.option = option or "-pn_linear_" + key
        self.always, self.class_key = always, class_key
        self.call_fwd, self.call_bwd = call_fwd, call_bwd
        self.capability = "linear_" + key if flagged else None
        self.bwd_entry, self.bwd_kernel = bwd_entry, bwd_kernel
        self.saves_pre = saves_pre
        self.torch_fwd, self.fwd = torch_fwd, fwd
        self.gz_text, self.gz, self.gz_bar = gz_text, gz, gz_bar
        self.torch_bwd = gz_text + " + matmul"
        self.check = check
        self.says, self.legacy = says, legacy
        # the wording of the status and of the forward check's warning
        self.none = none or "no eligible Linear -> %s pair" % self.name
        self.plural = plural
        self.fwd_off = fwd_off or "the fused Linear -> %s forward is switched off for this solver: " % self.name


KINDS = (
    # g_z to 3 * 2^-24 |g|: two roundings in 1 - a^2, one in the product, with or without an fma
    _Kind("tanh", nn.Tanh, "torch.tanh(F.linear)", torch.tanh, "tanh_backward", torch.ops.aten.tanh_backward, 3.0, _relative,
          _legacy("", _FLAGS + ("bwd_mode",), plans="plans", count="fused"), option="-pn_linear_fwd", always=True, class_key=True,
          call_fwd=_fwd_tanh, call_bwd=_bwd_tanh, flagged=False, bwd_kernel="pn_linear_bwd"),
    # g_z bit for bit: the kernel does no arithmetic on it
    _Kind("relu", nn.ReLU, "torch.relu(F.linear)", torch.relu, "threshold_backward", _relu_gz, None, _relative,
          _legacy("relu", _FLAGS + ("active", "status"), plans="relu")),
    # g_z to 1.5 * 2^-24 |g|: two roundings here, three in sigmoid_backward, each relative to |g a (1 - a)| <= |g| / 4
    _Kind("sigmoid", nn.Sigmoid, "torch.sigmoid(F.linear)", torch.sigmoid, "sigmoid_backward", torch.ops.aten.sigmoid_backward, 1.5,
          _barred, _legacy("sigmoid", ("active", "status"), plans="sigmoid", record="sig"), says=("refused",)),
    # g_z to 32 * 2^-24 |g|, ABSOLUTE in the derivative d = cdf + z pdf, which crosses zero near z = -0.7518 (a bar relative to |g d|
    # would be 0 there): each side evaluates erff once, within the 16 ulp OpenCL allows erf, of a value up to 1, halved in cdf --
    # 8 * 2^-24 a side; z pdf <= 0.25 adds less than one more; twice that for the two sides
    _Kind("gelu", nn.GELU, "F.gelu(F.linear)", F.gelu, "gelu_backward", _gelu_gz, 32.0, _barred,
          _legacy("gelu", ("active", "status"), record="gelu"), param_why=_gelu_why, call_fwd=_fwd_pre, saves_pre=True,
          says=("static", "refused")),
    # g_z to 4 * 2^-24 |g|: either side's expm1 is held to that of the exact g (1 - e^-a) (the kernel's by its GPU test), and they are
    # the same function of the same library
    _Kind("softplus", nn.Softplus, "F.softplus(F.linear)", F.softplus, "g * (-expm1(-a))", _softplus_gz, 4.0, _barred,
          _legacy("softplus", ("status",), record="softplus"), param_why=_softplus_why, says=("static", "refused")),
    # g_z to 1.5 * 2^-24 |g|: one rounded add, one rounded product on both sides
    _Kind("elu", nn.ELU, "F.elu(F.linear)", F.elu, "elu_backward", _elu_gz, 1.5, _barred,
          _legacy("elu", ("status",), record="elu"), param_why=_elu_why, says=("static", "refused")),
    # the bare layer: no activation, so no g_z -- its backward check is _check_bare_bwd
    _Kind("bare", nn.Linear, "F.linear", _identity, "", None, None, _relative,
          _legacy("bare", _FLAGS + ("active", "status"), plans="bare"), call_fwd=_fwd_bare, call_bwd=_bwd_bare, flagged=False,
          bwd_entry="linear_dx", bwd_kernel="pn_linear_dx", none="no eligible bare layer", plural="layers",
          fwd_off="the bare Linear layers run the stock modules for this solver: "),
)
PAIRS, BARE = KINDS[:-1], KINDS[-1]


def _find(func, params, kinds):
    """find_layers for the rows `kinds` of PAIRS: ([(sequential, {index of the Linear child: (linear, activation, row)})], {(row, class
    name of a container): reason}, bare)."""
    plans, refused, bare = [], {}, []
    if not isinstance(func, nn.Module):
        return plans, refused, bare
    index = {id(p) for p in params}
    owners = {}
    for m in func.modules():
        for p in m._parameters.values():
            if p is not None:
                owners[id(p)] = owners.get(id(p), 0) + 1
    seen = set()
    for seq in func.modules():
        if not isinstance(seq, nn.Sequential) or id(seq) in seen:
            continue
        seen.add(id(seq))
        kids = list(seq._modules.values())
        pairs = {}
        for i in range(len(kids) - 1):
            lin, act = kids[i], kids[i + 1]
            if not isinstance(lin, nn.Linear):
                continue
            kind = next((k for k in kinds if isinstance(act, k.module)), None)
            if kind is None:
                continue
            why = _static_why(seq, kids, lin, act, index, owners, kind.module)
            if why is None and kind.param_why is not None:
                why = kind.param_why(act)
            if why is None:
                pairs[i] = (lin, act, kind)
            else:
                refused.setdefault((kind, type(seq).__name__), why)
        if pairs:
            plans.append((seq, pairs))
        alone = {i: m for i, m in enumerate(kids)
                 if type(m) is nn.Linear and i not in pairs and _static_why(seq, kids, m, None, index, owners) is None}
        if alone:
            bare.append((seq, alone))
    return plans, refused, bare


def find_layers(func, params, relu=False, sigmoid=False, gelu=False, softplus=False, elu=False):
    """(plans, refused, bare): [(sequential, {index of the Linear child: (linear, activation)})] of func, the pairs of every kind that
    is looked for -- Linear -> Tanh always, every other row of PAIRS with its keyword (its option is 1), told apart by their second
    member; {key: reason} for the pairs that cannot be owned (what -pn_linear_fwd 1 warns about), the key the class name of the
    container for a tanh pair and (class name, "ReLU") ... (class name, "ELU") for the others, also for a module with parameters the
    kernel has no slot for (nn.GELU(approximate='tanh'), nn.Softplus(beta=2)); and [(sequential, {index of the child: linear})] for
    the bare layers -- exactly nn.Linear, opening no pair that is looked for, under the same static rules (-pn_linear_bare 1)."""
    on = dict(relu=relu, sigmoid=sigmoid, gelu=gelu, softplus=softplus, elu=elu)
    found, refused, bare = _find(func, params, [k for k in PAIRS if k.always or on[k.key]])
    plans = [(seq, {i: p[:2] for i, p in pairs.items()}) for seq, pairs in found]
    return plans, {(cls if kind.class_key else (cls, kind.name)): why for (kind, cls), why in refused.items()}, bare


def find_pairs(func, params):
    """The first two of find_layers."""
    return find_layers(func, params)[:2]


class _Call(object):
    """What one fused call carries into its backward.  state: the record of its kind; pre: the call also writes the pre-activation."""
    __slots__ = ("owner", "module", "grads", "ev", "version", "pre", "state")


class _PairState(object):
    """One kind of owned layer in one solver: the fields of its row of KINDS (`kind`) and, beside them, everything that changes."""
    def __init__(self, kind):
        self.kind = kind
        self.__dict__.update(vars(kind))
        self.plans = []            # [(sequential, {child index: (linear, activation)})]; the bare layers: {child index: linear}
        self.mode = "auto" if kind.always else "0"
        self.bwd_mode = "auto"     # -pn_linear_bwd, which governs every kind's backward: the tanh record's holds it
        self.disabled = False      # the forward check failed
        self.why = None
        self.checked = False
        self.n = 0                 # calls that ran as one launch
        self.n_pre = 0             # ... those of them that also wrote the pre-activation (pn_linear_fwd_pre; `saves_pre`)
        self.static_why = None     # why a pair of this kind is none (find_layers' `refused`), for the status
        self.bwd_disabled = False  # the backward check failed (the forward stays)
        self.bwd_why = None
        self.bwd_checked = False
        self.n_bwd = 0             # backwards that ran as one launch
        self.warned = False
        self.warned_bwd = False
        self.refused = None        # the reason of the last call-time refusal (LinearFwd._fusable): that call ran the stock modules

    @property
    def active(self):
        return (self.always or self.mode == "1") and bool(self.plans) and not self.disabled

    @property
    def n_y(self):
        """Calls that ran the y-only form: nobody differentiates them."""
        return self.n - self.n_pre

    @property
    def status(self):
        if not (self.always or self.mode == "1"):
            return "off (%s 0)" % self.option
        if not self.plans:
            return "stock modules (%s%s)" % (self.none, "" if "static" not in self.says or self.static_why is None else ": " + self.static_why)
        if self.disabled:
            return "stock modules (%s)" % self.why
        return "fused (%d %s; %d forward, %d backward calls so far%s)" % (
            sum(len(p) for _, p in self.plans), self.plural, self.n, self.n_bwd,
            "" if "refused" not in self.says or self.refused is None else "; the stock modules where a call is refused, last: " + self.refused)


def _shaped(y2, shape):
    """The kernel's (rows, out_f) result in the shape of the layer's output.  A 2-D input gets the tensor itself: a view made inside a
    Function's forward may not be written in place, and an nn.ReLU(inplace=True) behind a bare layer does just that."""
    return y2 if y2.shape == shape else y2.view(shape)


class _LinearTanh(torch.autograd.Function):
    """A pair of any kind (call.state: its record; the name is the first kind's).  Saved: (x, w, s), s the pair's output or, for a
    kind that `saves_pre`, the pre-activation from the same launch when somebody will differentiate the call (call.pre) -- the output
    is then not saved -- and nothing when nobody will."""
    @staticmethod
    def forward(ctx, x, w, b, call):
        st = call.state
        x2 = x.reshape(-1, w.shape[1])
        shape = x.shape[:-1] + (w.shape[0],)
        z2 = torch.empty((x2.shape[0], w.shape[0]), dtype=x2.dtype, device=x2.device) if call.pre else None
        a = _shaped(call.owner.kernel(st, x2, w, b, z2), shape)
        if call.pre:
            ctx.save_for_backward(x, w, _shaped(z2, shape))
        elif not st.saves_pre:
            ctx.save_for_backward(x, w, a)
        ctx.call = call
        ctx.has_bias = b is not None
        return a

    @staticmethod
    def backward(ctx, g):
        x, w, s = ctx.saved_tensors
        call = ctx.call
        # both in one launch where LinearFwd._bwd_fusable allows it, else the two torch operations
        fused = call.owner._backward(call.state, g, s, w) if ctx.needs_input_grad[0] else None
        if fused is not None:
            g_z, dx = fused
        else:
            g_z = call.state.gz(g, s)
            dx = torch.matmul(g_z, w) if ctx.needs_input_grad[0] else None
        dw, db = _param_grads(ctx, call, g_z, x, w)
        return dx, dw, db, None


def _param_grads(ctx, call, g_z, x, w):
    """(dW, db) of the Linear of one fused call for autograd, or (None, None) after handing (g_z, x) to the engine."""
    lg, ev = call.grads, call.ev
    taken = False
    if lg is not None and ev is not None and id(call.module) in lg.slots and not (lg.muted or lg.disabled or ev.muted):
        # the path of a hooked layer's output hook (pnode_amd/_lineargrad.py): queued for the stage's grouped launch
        lg._grad_hook(call.module, x.detach(), call.version, ev, g_z)
        taken = not lg.disabled              # (a backward pass that is not a stage VJP of the solver switches the engine off there)
    dw = db = None
    if not taken:
        g2 = g_z.reshape(-1, w.shape[0])
        if ctx.needs_input_grad[1]:
            dw = g2.t().mm(x.reshape(-1, w.shape[1]))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g2.sum(0)
    return dw, db


class _Linear(torch.autograd.Function):
    """A bare layer (-pn_linear_bare 1): _LinearTanh without the activation."""
    @staticmethod
    def forward(ctx, x, w, b, call):
        y = _shaped(call.owner.kernel(call.state, x.reshape(-1, w.shape[1]), w, b, None), x.shape[:-1] + (w.shape[0],))
        ctx.save_for_backward(x, w)
        ctx.call = call
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        call = ctx.call
        dx = None
        if ctx.needs_input_grad[0]:
            # pn_linear_dx where LinearFwd._bwd_fusable allows it, else the torch operation
            dx = call.owner._backward_bare(g, w)
            if dx is None:
                dx = torch.matmul(g, w)
        dw, db = _param_grads(ctx, call, g, x, w)
        return dx, dw, db, None


class LinearFwd(object):
    """The records of one solver (`records`: {key: _PairState}, in the order of KINDS) and the code that runs them.  The names the
    records' fields have had on this object -- `plans`, `n_fused`, `relu_disabled`, `sig`, `gelu_status` ... -- read them (`legacy`)."""
    device_type = "cuda"           # (the tests of the eligibility rules run the rules on host tensors)

    def __init__(self, ode):
        self._ode = weakref.ref(ode)
        self.records = {kind.key: _PairState(kind) for kind in KINDS}
        self._tanh, self._bare_st = self.records["tanh"], self.records[BARE.key]
        self._ok = {}              # (rows, out_f, in_f) -> pn_linear_fwd_supported
        self._ok_bwd = {}          # (entry, rows, out_f, in_f) -> pn_<entry>_supported

    def install(self, func, params, mode="auto", bwd_mode="auto", bare_mode="0", relu_mode="0", sigmoid_mode="0", gelu_mode="0",
                softplus_mode="0", elu_mode="0"):
        """Find the eligible pairs of `func` (the tanh pairs, and those of every kind whose mode is "1") and its bare layers; returns
        True when there is at least one that will run fused."""
        modes = dict(tanh=mode, bare=bare_mode, relu=relu_mode, sigmoid=sigmoid_mode, gelu=gelu_mode, softplus=softplus_mode, elu=elu_mode)
        for st in self.records.values():
            st.mode, st.plans, st.refused, st.static_why = modes[st.key], [], None, None
        self._tanh.bwd_mode = bwd_mode
        found, refused, self._bare_st.plans = _find(func, params, [k for k in PAIRS if k.always or modes[k.key] == "1"])
        for seq, pairs in found:
            for st in self.records.values():
                mine = {i: p[:2] for i, p in pairs.items() if p[2] is st.kind}
                if mine:
                    st.plans.append((seq, mine))
        told = []
        for (kind, cls), why in refused.items():
            st = self.records[kind.key]
            if st.static_why is None:
                st.static_why = why
            if mode == "1" and not st.warned:
                told.append(st)
                warnings.warn("pnode_amd: -pn_linear_fwd 1: a Linear -> %s pair of %s runs the stock modules: %s" % (st.name, cls, why), RuntimeWarning)
        for st in told:
            st.warned = True
        return self.active or bool(self.plans)

    @property
    def active(self):
        return any(st.active for st in self.records.values())

    @property
    def kinds(self):
        """The Softplus and the ELU record (what the name held when only those two were told by their record)."""
        return self.softplus, self.elu

    def _state(self, act):
        """The record of the pairs whose activation is exactly of `act`'s class, or None."""
        return next((st for st in self.records.values() if type(act) is st.module and st.kind is not BARE), None)

    def kernel(self, st, x2, w, b, z):
        return st.call_fwd(self._ode()._ops, st.key, x2, w, b, z)

    def kernel_bwd(self, st, g2, s2, w):
        return st.call_bwd(self._ode()._ops, st.key, g2, s2, w)

    def supported(self, rows, out_f, in_f):
        key = (rows, out_f, in_f)
        ok = self._ok.get(key)
        if ok is None:
            ops = self._ode()._ops
            ok = self._ok[key] = bool(hasattr(ops, "linear_fwd_supported") and ops.linear_fwd_supported(rows, out_f, in_f))
        return ok

    def _refuse(self, st, why):
        if self._tanh.mode == "1" and not st.warned:
            st.warned = True
            warnings.warn("pnode_amd: -pn_linear_fwd 1: a Linear -> %s pair runs the stock modules: %s" % (st.name, why), RuntimeWarning)

    def _fusable(self, lin, x):
        """The call-time half of the eligibility rules; None or the reason as a string."""
        ode = self._ode()
        if ode is None or not isinstance(x, torch.Tensor):
            return "the input is no tensor"
        w, b = lin.weight, lin.bias
        if _autocast_on(x.device.type):
            return "autocast is on"
        if x.device.type != self.device_type or x.dtype != torch.float32 or x.dtype != ode.tensor_dtype or w.dtype != torch.float32 or (b is not None and b.dtype != torch.float32):
            return "not a CUDA fp32 tensor of the state's dtype"
        if x.dim() < 1 or x.shape[-1] != w.shape[1] or not x.is_contiguous() or not w.is_contiguous() or (b is not None and not b.is_contiguous()):
            return "operands are not contiguous"
        if w.device != x.device or x.data_ptr() % 16 or w.data_ptr() % 16:
            return "operands are not 16-byte aligned on one device"
        if not self.supported(x.numel() // w.shape[1], w.shape[0], w.shape[1]):
            return "outside pn_linear_fwd_supported"
        return None

    def _check(self, st, x, w, b, a, z=None):
        """First fused call of a kind in a solver: through torch as well, in the form of the kind's `check` (_relative, _barred), `z`
        the pre-activation where the call wrote it.  True, or False after switching off that kind's forward -- only it."""
        st.checked = True
        with torch.no_grad():
            x2 = x.reshape(-1, w.shape[1])
            lin = F.linear(x2, w, b)
            ref = st.fwd(lin)
            scale = x2.abs() @ w.abs().t()
            if b is not None:
                scale = scale + b.abs()
            judged, why = st.check(st, a.reshape(ref.shape), ref, z, lin, scale)
        if not judged:
            st.checked = False                     # nothing to judge by: the next call is checked
        if why is not None:
            st.disabled, st.why = True, why
            warnings.warn("pnode_amd: " + st.fwd_off + why, RuntimeWarning)
        return why is None

    # ---- the backward of a pair (called from _LinearTanh.backward)
    def supported_bwd(self, rows, out_f, in_f, entry="linear_bwd"):
        key = (entry, rows, out_f, in_f)
        ok = self._ok_bwd.get(key)
        if ok is None:
            ops = self._ode()._ops
            ok = self._ok_bwd[key] = bool(hasattr(ops, entry + "_supported") and getattr(ops, entry + "_supported")(rows, out_f, in_f))
        return ok

    def _bwd_fusable(self, st, g, s, w):
        """None, or the reason (a string) this backward of a layer of `st` runs the torch operations.  s: the tensor the pair saved; None
        for a bare layer (pn_linear_dx: the same rules minus everything about s)."""
        ode = self._ode()
        if ode is None or not hasattr(ode._ops, st.bwd_entry):
            return "the backend has no " + st.bwd_entry
        if st.capability is not None and not getattr(ode._ops, st.capability, False):
            return "the backend has no " + st.capability
        if self._tanh.bwd_mode == "0":
            return "-pn_linear_bwd 0"
        if st.bwd_disabled:
            return st.bwd_why
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != w.device or g.device.type != self.device_type \
                or (g.dim() < 1 or g.shape[-1] != w.shape[0] if s is None else g.shape != s.shape):
            return "the cotangent is no fp32 tensor of the pair's shape on the weight's device"
        if not (g.is_contiguous() and (s is None or s.is_contiguous()) and w.is_contiguous()):
            return "the cotangent is not contiguous"
        if g.data_ptr() % 16 or (s is not None and s.data_ptr() % 16) or w.data_ptr() % 16:
            return "operands are not 16-byte aligned"
        if _autocast_on(g.device.type):
            return "autocast is on"
        if torch.is_grad_enabled():
            return "the backward pass is itself differentiated (create_graph)"
        if not self.supported_bwd(g.numel() // w.shape[0], w.shape[0], w.shape[1], st.bwd_entry):
            return "outside pn_%s_supported" % st.bwd_entry
        return None

    def _check_bwd(self, st, g2, s2, w, gz, dx):
        """First fused backward of a kind in a solver: both results through torch as well.  gz to st.gz_bar * 2^-24 |g| of st.gz(g, s),
        elementwise (the bars: KINDS), or, with no bar, bit for bit -- then a g_z that differs is a miss even with no cell of dx to
        judge by; dx to CHECK_TOL of |gz| |w| (the forward's bar in the forward's measure).  Returns None, or the torch results after
        switching that kind's fused backward -- only it -- off."""
        st.bwd_checked = True
        gz_t = st.gz(g2, s2)
        dx_t = torch.matmul(gz_t, w)
        scale = gz_t.abs() @ w.abs()
        ok = torch.isfinite(dx_t) & (scale > 0)
        some = bool(ok.any())
        if st.gz_bar is None:
            bad_z, miss = not torch.equal(gz.view(torch.int32), gz_t.view(torch.int32)), "g_z is not %s's bit for bit" % st.gz_text
            judged = bad_z or some
        else:
            fin = torch.isfinite(gz_t)
            judged, miss = some and bool(fin.any()), "g_z by more than %g * 2^-24 |g|" % st.gz_bar
            bad_z = judged and bool((~((gz - gz_t).abs() <= st.gz_bar * 2.0 ** -24 * g2.abs()) & fin).any())
        if not judged:
            st.bwd_checked = False                 # nothing to judge by: the next call is checked
            return None
        err = float(((dx - dx_t).abs() / scale)[ok].max()) if some else 0.0
        if bad_z or not err <= CHECK_TOL:
            st.bwd_disabled = True
            st.bwd_why = "%s and %s differ: " % (st.bwd_kernel, st.torch_bwd) + (
                miss if bad_z else "dx by %.2e of |g_z| |w| (allowed: %.0e)" % (err, CHECK_TOL))
            warnings.warn("pnode_amd: the fused Linear -> %s backward is switched off for this solver: %s" % (st.name, st.bwd_why), RuntimeWarning)
            return gz_t, dx_t
        return None

    def _backward(self, st, g, s, w):
        """(g_z, dx) of one pair of `st` in one launch (s: the tensor the pair saved), or None: the caller runs st.gz and matmul."""
        why = self._bwd_fusable(st, g, s, w)
        if why is not None:
            if self._tanh.bwd_mode == "1" and not st.warned_bwd:
                st.warned_bwd = True
                warnings.warn("pnode_amd: -pn_linear_bwd 1: the backward of a Linear -> %s pair runs the torch operations: %s"
                              % (st.name, why), RuntimeWarning)
            return None
        out_f, in_f = w.shape
        g2, s2 = g.reshape(-1, out_f), s.reshape(-1, out_f)
        with torch.no_grad():
            gz, dx = self.kernel_bwd(st, g2, s2, w)
            if not st.bwd_checked and not (g.is_cuda and torch.cuda.is_current_stream_capturing()):
                torch_way = self._check_bwd(st, g2, s2, w, gz, dx)
                if torch_way is not None:
                    gz, dx = torch_way
                    return gz.view(g.shape), dx.view(g.shape[:-1] + (in_f,))
        st.n_bwd += 1
        return gz.view(g.shape), dx.view(g.shape[:-1] + (in_f,))

    # ---- the backward of a bare layer (called from _Linear.backward)
    def _check_bare_bwd(self, st, g2, w, dx):
        """First pn_linear_dx of a solver: through torch as well, to CHECK_TOL of |g| |w| (the pair's bar in the pair's measure).  Returns
        None, or the torch result after switching the bare backward -- only it -- off."""
        st.bwd_checked = True
        dx_t = torch.matmul(g2, w)
        scale = g2.abs() @ w.abs()
        ok = torch.isfinite(dx_t) & (scale > 0)
        if not bool(ok.any()):
            st.bwd_checked = False                 # nothing to judge by: the next call is checked
            return None
        err = float(((dx - dx_t).abs() / scale)[ok].max())
        if not err <= CHECK_TOL:
            st.bwd_disabled = True
            st.bwd_why = "pn_linear_dx and matmul differ: dx by %.2e of |g| |w| (allowed: %.0e)" % (err, CHECK_TOL)
            warnings.warn("pnode_amd: the backward of the bare Linear layers runs matmul for this solver: " + st.bwd_why, RuntimeWarning)
            return dx_t
        return None

    def _backward_bare(self, g, w):
        """dx of one bare layer by pn_linear_dx, or None: the caller runs matmul."""
        st = self._bare_st
        if self._bwd_fusable(st, g, None, w) is not None:
            return None
        out_f, in_f = w.shape
        g2 = g.reshape(-1, out_f)
        with torch.no_grad():
            dx = self.kernel_bwd(st, g2, None, w)
            if not st.bwd_checked and not (g.is_cuda and torch.cuda.is_current_stream_capturing()):
                torch_way = self._check_bare_bwd(st, g2, w, dx)
                if torch_way is not None:
                    return torch_way.view(g.shape[:-1] + (in_f,))
        st.n_bwd += 1
        return dx.view(g.shape[:-1] + (in_f,))

    @property
    def bwd_status(self):
        st = self._tanh
        if st.bwd_mode == "0":
            return "torch operations (-pn_linear_bwd 0)"
        ode = self._ode()
        if ode is None or not hasattr(ode._ops, st.bwd_entry):
            return "torch operations (the backend has no %s)" % st.bwd_entry
        if st.bwd_disabled:
            return "torch operations (%s)" % st.bwd_why
        return "fused (%d calls so far)" % st.n_bwd

    def _call(self, st, lin, x, grads):
        """(the _Call of one fused call of `lin`, the evaluation that records it or None)."""
        ev = grads.recording if grads is not None else None
        if ev is not None and not grads.note_fused(lin, x):
            ev = None                             # (the evaluation is left to autograd: LinearParamGrads.end mutes it)
        call = _Call()
        call.owner, call.module, call.grads, call.ev, call.version, call.state, call.pre = self, lin, grads, ev, x._version, st, False
        return call, ev

    def _pair(self, st, lin, act, x, grads):
        """One pair of `st`: Linear -> `act` (the activation's module is not called)."""
        why = self._fusable(lin, x)
        if why is not None:
            st.refused = why
            self._refuse(st, why)
            return act(lin(x))
        w, b = lin.weight, lin.bias
        call, ev = self._call(st, lin, x, grads)
        if st.saves_pre:
            # the saved-pre-activation form only where somebody will differentiate the call: else y alone, and no z is allocated
            call.pre = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad))
        a = _LinearTanh.apply(x, w, b, call)
        if not st.checked and not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            z = a.grad_fn.saved_tensors[2] if call.pre and a.grad_fn is not None else None
            if not self._check(st, x.detach(), w.detach(), None if b is None else b.detach(), a.detach(), z):
                return act(lin(x))
        if ev is not None and a.grad_fn is not None:
            ev.through[a.grad_fn] = x.grad_fn     # Evaluation.clean passes the pair along its input edge only
        st.n += 1
        st.n_pre += 1 if call.pre else 0
        return a

    def _bare(self, lin, x, grads):
        """One bare layer (-pn_linear_bare 1): _pair without the activation."""
        st = self._bare_st
        if self._fusable(lin, x) is not None:
            return lin(x)
        w, b = lin.weight, lin.bias
        call, ev = self._call(st, lin, x, grads)
        y = _Linear.apply(x, w, b, call)
        if not st.checked and not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            if not self._check(st, x.detach(), w.detach(), None if b is None else b.detach(), y.detach()):
                return lin(x)
        if ev is not None and y.grad_fn is not None:
            ev.through[y.grad_fn] = x.grad_fn     # Evaluation.clean passes the layer along its input edge only
        st.n += 1
        return y

    def _runner(self, seq, pairs, alone, grads):
        bare = self._bare_st

        def forward(inp):
            kids = list(seq._modules.values())
            i, n = 0, len(kids)
            while i < n:
                p = pairs.get(i)
                if p is not None and i + 1 < n and kids[i] is p[0] and kids[i + 1] is p[1] and not p[2].disabled:
                    inp = self._pair(p[2], p[0], p[1], inp, grads)
                    i += 2
                elif alone.get(i) is kids[i] and not bare.disabled:
                    inp = self._bare(kids[i], inp, grads)
                    i += 1
                else:
                    inp = kids[i](inp)
                    i += 1
            return inp
        return forward

    def _containers(self):
        """[(sequential, {child index: (linear, activation, record)}, its bare layers)]: the pairs of every kind that is active, the bare
        layers with -pn_linear_bare 1."""
        out = {}
        for st in self.records.values():
            if not st.active:
                continue
            for seq, plan in st.plans:
                _, pairs, alone = out.setdefault(id(seq), (seq, {}, {}))
                if st is self._bare_st:
                    alone.update(plan)
                else:
                    pairs.update((i, p + (st,)) for i, p in plan.items())
        return list(out.values())

    @contextlib.contextmanager
    def window(self, grads=None):
        """The solver evaluates func: until the window closes the eligible containers run their pairs fused.  `grads`: the
        solver's LinearParamGrads when it records this evaluation, else None."""
        put = []
        try:
            if self.active and not _global_hooks():
                for seq, pairs, alone in self._containers():
                    if "forward" in seq.__dict__ or type(seq) is not nn.Sequential:
                        continue
                    if _user_hooked(seq) or any(_user_hooked(m) for pr in pairs.values() for m in pr[:2]):
                        for st in self.records.values():
                            if any(pr[2] is st for pr in pairs.values()):
                                self._refuse(st, "a forward, pre-forward or backward hook on the pair or its container")
                        if _user_hooked(seq):
                            continue
                        pairs = {}                # (a hooked pair keeps the stock modules; the bare layers of the container stay)
                    alone = {i: m for i, m in alone.items() if not _user_hooked(m)}
                    if not pairs and not alone:
                        continue
                    seq.__dict__["forward"] = self._runner(seq, pairs, alone, grads)
                    put.append(seq)
            yield
        finally:
            for seq in put:
                seq.__dict__.pop("forward", None)


def _reader(key, field):
    if field is None:
        return property(lambda self: self.records[key])
    return property(lambda self: getattr(self.records[key], field))


for _kind in KINDS:
    for _name, _field in _kind.legacy.items():
        setattr(LinearFwd, _name, _reader(_kind.key, _field))
