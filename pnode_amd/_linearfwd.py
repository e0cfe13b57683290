"""func's ``nn.Linear -> nn.Tanh`` pairs as ONE launch in the solver's own evaluations of func (``pn_linear_fwd``, csrc/pn_linear.hip).

The body of ``evalRHSFunction`` (pa.py:393-412) at BASELINE's target configuration is four library GEMMs and three elementwise
``tanh`` launches; each ``tanh`` moves 16 MiB in about 6 us, twice what its traffic needs -- mostly dispatch floor.  A pair is
therefore run as one MFMA kernel with the bias and ``tanhf`` in its epilogue, where ALL of this holds:

* the pair is two consecutive children of an ``nn.Sequential`` whose ``forward`` is ``nn.Sequential``'s own; the first is exactly
  ``nn.Linear`` (no subclass; weight and bias trainable parameters of the solver, owned by no other module -- the rules of
  ``LinearParamGrads.install``), the second exactly ``nn.Tanh``;
* neither module nor the container carries a hook that is not the engine's own, and no global module hook is registered;
* at call time: the input is a contiguous CUDA fp32 tensor of the state's dtype, autocast is off, ``pn_linear_fwd_supported``.

Anything else runs the stock modules.  Only evaluations inside ``LinearFwd.window`` are affected -- the solver opens it around its own
calls of func; for its duration the eligible containers carry an instance-level ``forward`` (the runner below), removed when the window
closes, also when func raises: func is left exactly as found (pnode_amd/_funcguard.py sees no change between two calls).

Autograd: the pair is one ``torch.autograd.Function``.  Its backward forms ``g_z = g_a (1 - a^2)`` and ``dx = g_z W`` in ONE launch
(``pn_linear_bwd``: the tanh' prologue in registers, W read as it lies) where the backend has ``linear_bwd``, ``-pn_linear_bwd`` is not
``0``, the input needs a gradient, ``g_a`` is a contiguous, 16-byte aligned fp32 tensor of the pair's shape on the weight's device,
autocast is off, the backward is not itself differentiated and ``pn_linear_bwd_supported``; otherwise with the torch operations
autograd runs for the stock modules (``tanh_backward``, ``matmul``).  A solver's first fused backward outside a capture is formed both
ways: ``g_z`` must agree to ``3 * 2^-24 |g_a|`` (two roundings in ``1 - a^2``, one in the product, with or without an fma) and ``dx``
to 1e-6 of ``|g_z| |W|``; a miss switches the fused BACKWARD off for that solver (the forward stays), ``bwd_why`` recorded, and the
torch results are returned.  Either way the backward hands ``(g_z, x)`` to
``LinearParamGrads._grad_hook`` (the queue, the grouped launch, the side stream, the deferral under per-evaluation graphs) when that
is active for the evaluation; otherwise it returns ``dW = g_z^T x`` and ``db = colsum(g_z)`` to autograd.  ``Evaluation.clean`` sees
the pair's node as it sees a hooked layer: the walk goes on along the input edge only.

At a solver's first fused evaluation outside a capture the pair is computed through torch as well; a difference above 1e-6 of
``sum |x w| + |b|`` (the library path's own 1.0e-7, the split product's 5.7e-8 and a few ulp of the two tanh, with room) switches
fusing off for that solver, ``why`` recorded.  ``-pn_linear_fwd auto|0|1``, ``-pn_linear_bwd auto|0|1``.

BARE layers (``-pn_linear_bare 0|1``, default ``0``: nothing below happens).  A child of an eligible container that is exactly
``nn.Linear``, opens no fused pair and passes the static rules of a pair's Linear (``_static_why``, the same code) is a bare layer: the
head of every ``... -> Linear`` net, a Linear in front of a ReLU or of a subclass of ``nn.Tanh``.  With ``1`` the runner sends it through
``_Linear``: forward ``pn_linear_fwd`` with the identity under the call-time rules of ``_fusable``; backward ``dx = g W`` by
``pn_linear_dx`` (the kernel body of ``pn_linear_bwd`` without the tanh' prologue: no ``a`` read, no ``g_z`` written) under the rules of
``_bwd_fusable`` minus everything about ``a``, else ``matmul``; ``(g, x)`` then goes to ``LinearParamGrads._grad_hook`` exactly as a
pair's ``(g_z, x)`` does.  A container whose only eligible members are bare layers is active too.  The self-checks are the pair's in
the pair's measures (forward against ``F.linear``, ``dx`` against ``matmul``); a miss switches off the bare path, or its backward,
only -- the pairs are not touched.  The bare layers are kept in ``LinearFwd.bare``, beside ``plans``.

ReLU pairs (``-pn_linear_relu 0|1``, default ``0``: nothing below happens, a Linear in front of a ReLU stays a stock module or a bare
layer).  With ``1`` two consecutive children ``nn.Linear``, exactly ``nn.ReLU`` (either ``inplace``: the module is not called) of an
eligible container are a pair under the static and hook rules of a tanh pair, kept in ``LinearFwd.relu``; such a Linear is no bare layer.
The pair runs through ``_LinearTanh`` with ``call.relu``: forward ``pn_linear_fwd`` with ``PN_ACT_RELU`` under ``_fusable``; backward
``g_z = threshold_backward(g, a, 0)`` and ``dx = g_z W`` in one launch (``pn_linear_bwd_act``) under ``_bwd_fusable`` on a backend with
``linear_relu``, else ``threshold_backward`` and ``matmul``; ``(g_z, x)`` goes to ``LinearParamGrads._grad_hook`` as a tanh pair's.
Self-checks of their own: the forward against ``torch.relu(F.linear)`` in the pair's measure; ``g_z`` must be ``threshold_backward``'s
bit for bit (the kernel does no arithmetic on it), ``dx`` in the pair's measure.  A miss switches off the ReLU pairs, or their backward,
only.  ``n_relu`` / ``n_relu_bwd`` count them; ``n_fused`` / ``n_fused_bwd`` stay the tanh pairs'.

Sigmoid pairs (``-pn_linear_sigmoid 0|1``, default ``0``: nothing below happens).  With ``1`` two consecutive children ``nn.Linear``,
exactly ``nn.Sigmoid`` of an eligible container are a pair under the same rules; such a Linear is no bare layer.  Their maps, flags and
counters are one record, ``LinearFwd.sig`` (a ``_PairState``), not a third copy of every field; ``n_sigmoid`` / ``n_sigmoid_bwd`` read
it.  The pair runs through ``_LinearTanh`` with ``call.sigmoid``: forward ``pn_linear_fwd`` with ``PN_ACT_SIGMOID``; backward
``g_z = g a (1 - a)`` and ``dx = g_z W`` in one launch (``pn_linear_bwd_act``) on a backend with ``linear_sigmoid``, else
``sigmoid_backward`` and ``matmul``.  The arithmetic is not exact, so the self-checks are bounds: the forward against
``torch.sigmoid(F.linear)`` to ``1e-6 (sum |x w| + |b|) + 4 * 2^-24`` -- the absolute term because a zero pre-activation maps to 0.5 with
a rounding of its own on either side (the kernel at most 2.5, the library about 1 ulp of 2^-24), where tanh and ReLU give an exact 0;
``g_z`` to ``1.5 * 2^-24 |g|`` of ``sigmoid_backward``'s (two roundings here, three there, relative to ``g a (1 - a) <= |g| / 4``); ``dx``
in the pairs' measure.  A miss switches off the Sigmoid pairs, or their backward, only.

GELU pairs (``-pn_linear_gelu 0|1``, default ``0``: nothing below happens): the SAVED PRE-ACTIVATION form.  The derivative of every
activation above is a function of the pair's output ``a``, so their Function saves ``(x, w, a)``.  GELU is not monotonic: its derivative
needs ``z = x W^T + b``, which cannot be had back from ``a``.  With ``1`` two consecutive children ``nn.Linear``, exactly ``nn.GELU`` with
``approximate == 'none'`` of an eligible container are a pair under the same rules (``approximate='tanh'`` is none: its reason is in
``refused`` under ``(class name, "GELU")`` and in the status); one record, ``LinearFwd.gelu``.  The pair runs through ``_LinearGelu``.
An evaluation that will be differentiated (grad mode on and the input or a parameter requires a gradient) launches ``pn_linear_fwd_pre``:
``y`` and ``z`` from one epilogue; ``(x, w, z)`` is saved and ``y`` is not -- the memory of the stock pair.  Any other evaluation (the
forward sweep without retained tapes) launches ``pn_linear_fwd`` with ``PN_ACT_GELU`` and allocates no ``z``.  ``LinearFwd.gelu.n``
counts both, ``n_pre`` the first kind, ``n_y`` the second.  Backward: ``g_z = g (cdf + z pdf)`` and ``dx = g_z W`` in one launch
(``pn_linear_bwd_act`` with ``PN_ACT_GELU``, reading ``z``) on a backend with ``linear_gelu``, else ``gelu_backward`` and ``matmul``.
Self-checks as the Sigmoid pairs': the forward against ``F.gelu(F.linear)`` to ``1e-6 (sum |x w| + |b|) + 4 * 2^-24`` (GELU crosses zero
at ``z = 0``: rows of scale 0 must have a bar above 0), ``z`` against ``F.linear`` in the bare layer's measure; ``g_z`` to ``32 * 2^-24 |g|``
of ``gelu_backward``'s -- absolute in the derivative, which crosses zero near ``z = -0.7518``: two evaluations of ``erff``, each within
the 16 ulp that OpenCL allows ``erf``, halved in ``cdf`` --; ``dx`` in the pairs' measure.  A miss switches off the GELU pairs, or their
backward, only.

Softplus and ELU pairs (``-pn_linear_softplus 0|1``, ``-pn_linear_elu 0|1``, default ``0``: nothing below happens).  Both derivatives are
functions of the pair's OUTPUT -- ``1 - e^-a`` and ``a > 0 ? 1 : a + 1`` --, so these are saved-output pairs through ``_LinearTanh``, one
record each (``LinearFwd.softplus``, ``LinearFwd.elu``) that also names the kernel's ``act``, the torch expressions the pair replaces and
the bar of ``g_z``: nothing about them is spelled per kind outside ``_KINDS``.  With ``1`` two consecutive children ``nn.Linear``, exactly
``nn.Softplus`` with ``beta == 1`` and ``threshold == 20`` (exactly ``nn.ELU`` with ``alpha == 1``, either ``inplace``: the module is not
called) of an eligible container are a pair under the rules of the Sigmoid pairs; a module with other parameters is none -- the C entries
have no slot for one --, its reason in ``refused`` under ``(class name, "Softplus")`` / ``(class name, "ELU")`` and in the status.  Forward
``pn_linear_fwd`` with ``PN_ACT_SOFTPLUS`` / ``PN_ACT_ELU``; backward one ``pn_linear_bwd_act`` launch on a backend with
``linear_softplus`` / ``linear_elu``, else ``g * (-expm1(-a))`` / ``aten.elu_backward(g, 1, 1, 1, True, a)`` and ``matmul``.  Self-checks:
the forward against ``F.softplus(F.linear)`` / ``F.elu(F.linear)`` at the Sigmoid pairs' bar (Softplus maps a zero pre-activation to
``log 2``: the absolute term again); ``g_z`` against those torch expressions to ``4 * 2^-24 |g|`` (Softplus: the cap on either side's
``expm1``) and ``1.5 * 2^-24 |g|`` (ELU: one rounded add, one rounded product); ``dx`` in the pairs' measure.  A miss switches off that
kind, or its backward, only."""
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
    """The static half of the eligibility rules for the Linear `lin` (and the activation `act` behind it, exactly a `kind`: nn.Tanh or
    nn.ReLU or nn.Sigmoid or nn.GELU or nn.Softplus or nn.ELU; None for a bare layer) among the children `kids` of `seq`: None, or the reason as a string."""
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


def _softplus_why(act):
    if act.beta != 1 or act.threshold != 20:
        return "nn.Softplus(beta=%r, threshold=%r): only beta == 1 and threshold == 20 are owned" % (act.beta, act.threshold)
    return None


def _elu_why(act):
    if act.alpha != 1.0:
        return "nn.ELU(alpha=%r): only alpha == 1 is owned" % (act.alpha,)
    return None


def find_layers(func, params, relu=False, sigmoid=False, gelu=False, softplus=False, elu=False):
    """(plans, refused, bare): [(sequential, {index of the Linear child: (linear, tanh)})] of func; {class name of a container: reason}
    for the Linear -> Tanh pairs that cannot be fused (what -pn_linear_fwd 1 warns about); and [(sequential, {index of the child:
    linear})] for the bare layers -- exactly nn.Linear, opening no fused pair, under the same static rules (-pn_linear_bare 1).
    relu (-pn_linear_relu 1): two consecutive children nn.Linear, nn.ReLU are a pair too, under the rules of a tanh pair -- (linear, relu)
    in `plans`, told from a tanh pair by its second member, and such a Linear is no bare layer; a ReLU pair that cannot be fused is in
    `refused` under the key (class name of the container, "ReLU").  Without it the three are what they were before there was the option.
    sigmoid (-pn_linear_sigmoid 1): the same for nn.Linear, nn.Sigmoid; the key in `refused` is (class name, "Sigmoid").
    gelu (-pn_linear_gelu 1): the same for nn.Linear, nn.GELU with approximate == 'none'; the key in `refused` is (class name, "GELU"),
    also for an nn.GELU(approximate='tanh'), whose Linear is then a stock module or a bare layer.
    softplus (-pn_linear_softplus 1), elu (-pn_linear_elu 1): the same for nn.Linear, nn.Softplus with beta == 1 and threshold == 20, and
    for nn.Linear, nn.ELU with alpha == 1; the keys in `refused` are (class name, "Softplus") and (class name, "ELU"), also for a module
    with other parameters."""
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
            if isinstance(act, nn.Tanh):
                kind, key = nn.Tanh, type(seq).__name__
            elif relu and isinstance(act, nn.ReLU):
                kind, key = nn.ReLU, (type(seq).__name__, "ReLU")
            elif sigmoid and isinstance(act, nn.Sigmoid):
                kind, key = nn.Sigmoid, (type(seq).__name__, "Sigmoid")
            elif gelu and isinstance(act, nn.GELU):
                kind, key = nn.GELU, (type(seq).__name__, "GELU")
            elif softplus and isinstance(act, nn.Softplus):
                kind, key = nn.Softplus, (type(seq).__name__, "Softplus")
            elif elu and isinstance(act, nn.ELU):
                kind, key = nn.ELU, (type(seq).__name__, "ELU")
            else:
                continue
            why = _static_why(seq, kids, lin, act, index, owners, kind)
            if why is None and kind is nn.GELU and getattr(act, "approximate", "none") != "none":
                why = "nn.GELU(approximate=%r): only the exact GELU (approximate='none') is owned" % (act.approximate,)
            if why is None and kind is nn.Softplus:
                why = _softplus_why(act)
            if why is None and kind is nn.ELU:
                why = _elu_why(act)
            if why is None:
                pairs[i] = (lin, act)
            else:
                refused.setdefault(key, why)
        if pairs:
            plans.append((seq, pairs))
        alone = {i: m for i, m in enumerate(kids)
                 if type(m) is nn.Linear and i not in pairs and _static_why(seq, kids, m, None, index, owners) is None}
        if alone:
            bare.append((seq, alone))
    return plans, refused, bare


def find_pairs(func, params):
    """The first two of find_layers."""
    return find_layers(func, params)[:2]


class _Call(object):
    """What one fused call carries into its backward."""
    __slots__ = ("owner", "module", "grads", "ev", "version", "relu", "sigmoid", "pre", "state")


class _PairState(object):
    """The state of one further kind of pair beside the tanh and ReLU pairs, whose fields are LinearFwd's own: the map, the option, the
    self-checks' flags and reasons, the counters.  `name` is the activation's class name, `torch_fwd` / `torch_bwd` the expressions the
    pair replaces (in the wording of the warnings)."""
    def __init__(self, name, option, torch_fwd, torch_bwd, kind=None, act=None, fwd=None, gz=None, gz_bar=None):
        self.name, self.option, self.torch_fwd, self.torch_bwd = name, option, torch_fwd, torch_bwd
        # the Softplus and ELU pairs (_KINDS): the module class, the backend's name of the activation, the torch functions behind
        # `torch_fwd` and `torch_bwd`'s first half -- fwd(z), gz(g, a) --, and the self-check's bar of g_z in units of 2^-24 |g|
        self.kind, self.act, self.fwd, self.gz, self.gz_bar = kind, act, fwd, gz, gz_bar
        self.plans = []            # [(sequential, {child index: (linear, activation)})]
        self.mode = "0"
        self.disabled = False      # the forward check failed
        self.why = None
        self.checked = False
        self.n = 0                 # pair calls that ran as one launch
        self.n_pre = 0             # ... those of them that also wrote the pre-activation (pn_linear_fwd_pre; the GELU pairs)
        self.static_why = None     # why a pair of this kind is none (find_layers' `refused`), for the status
        self.bwd_disabled = False  # the backward check failed (the forward stays)
        self.bwd_why = None
        self.bwd_checked = False
        self.n_bwd = 0             # pair backwards that ran as one launch (pn_linear_bwd_act)
        self.warned = False
        self.warned_bwd = False
        self.refused = None        # the reason of the last call-time refusal (LinearFwd._fusable): that call ran the stock modules

    @property
    def active(self):
        return self.mode == "1" and bool(self.plans) and not self.disabled

    @property
    def n_y(self):
        """Pair calls that ran the y-only form: nobody differentiates them."""
        return self.n - self.n_pre

    @property
    def status(self):
        if self.mode != "1":
            return "off (%s 0)" % self.option
        if not self.plans:
            return "stock modules (no eligible Linear -> %s pair%s)" % (self.name, "" if self.static_why is None else ": " + self.static_why)
        if self.disabled:
            return "stock modules (%s)" % self.why
        return "fused (%d pairs; %d forward, %d backward calls so far%s)" % (
            sum(len(p) for _, p in self.plans), self.n, self.n_bwd,
            "" if self.refused is None else "; the stock modules where a call is refused, last: " + self.refused)


def _softplus_gz(g, a):
    return g * (-torch.expm1(-a))


def _elu_gz(g, a):
    return torch.ops.aten.elu_backward(g, 1, 1, 1, True, a)


def _KINDS():
    """The records of the saved-output pairs that are told by their record alone (LinearFwd.softplus, LinearFwd.elu), fresh ones."""
    return (_PairState("Softplus", "-pn_linear_softplus", "F.softplus(F.linear)", "g * (-expm1(-a)) + matmul", nn.Softplus, "softplus",
                       F.softplus, _softplus_gz, 4.0),
            _PairState("ELU", "-pn_linear_elu", "F.elu(F.linear)", "elu_backward + matmul", nn.ELU, "elu", F.elu, _elu_gz, 1.5))


def _shaped(y2, shape):
    """The kernel's (rows, out_f) result in the shape of the layer's output.  A 2-D input gets the tensor itself: a view made inside a
    Function's forward may not be written in place, and an nn.ReLU(inplace=True) behind a bare layer does just that."""
    return y2 if y2.shape == shape else y2.view(shape)


class _LinearTanh(torch.autograd.Function):
    """A Linear -> Tanh pair or, with call.relu (-pn_linear_relu 1), a Linear -> ReLU pair, or, with call.sigmoid (-pn_linear_sigmoid 1), a
    Linear -> Sigmoid pair, or, with call.state (a record of _KINDS: -pn_linear_softplus 1, -pn_linear_elu 1), a Linear -> Softplus or
    Linear -> ELU pair: the same structure, the other activation."""
    @staticmethod
    def forward(ctx, x, w, b, call):
        if call.state is not None:
            a2 = call.owner.kernel_act(call.state.act, x.reshape(-1, w.shape[1]), w, b)
        else:
            kernel = call.owner.kernel_sigmoid if call.sigmoid else (call.owner.kernel_relu if call.relu else call.owner.kernel)
            a2 = kernel(x.reshape(-1, w.shape[1]), w, b)
        a = _shaped(a2, x.shape[:-1] + (w.shape[0],))
        ctx.save_for_backward(x, w, a)
        ctx.call = call
        ctx.has_bias = b is not None
        return a

    @staticmethod
    def backward(ctx, g):
        x, w, a = ctx.saved_tensors
        call = ctx.call
        # both in one launch (pn_linear_bwd, pn_linear_bwd_act) where LinearFwd._bwd_fusable allows it, else the two torch operations
        if not ctx.needs_input_grad[0]:
            fused = None
        elif call.state is not None:
            fused = call.owner._backward(g, a, w, st=call.state)
        elif call.sigmoid:
            fused = call.owner._backward(g, a, w, sigmoid=True)
        else:
            fused = call.owner._backward(g, a, w, call.relu)
        if fused is not None:
            g_z, dx = fused
        else:
            if call.state is not None:
                g_z = call.state.gz(g, a)
            elif call.sigmoid:
                g_z = torch.ops.aten.sigmoid_backward(g, a)
            else:
                g_z = torch.ops.aten.threshold_backward(g, a, 0) if call.relu else torch.ops.aten.tanh_backward(g, a)
            dx = torch.matmul(g_z, w) if ctx.needs_input_grad[0] else None
        dw, db = _param_grads(ctx, call, g_z, x, w)
        return dx, dw, db, None


class _LinearGelu(torch.autograd.Function):
    """A Linear -> GELU pair (-pn_linear_gelu 1): the sibling of _LinearTanh that saves the PRE-activation.  call.pre: somebody will
    differentiate this evaluation -- y and z from one launch, (x, w, z) saved, y not; else y alone and nothing saved."""
    @staticmethod
    def forward(ctx, x, w, b, call):
        y2, z2 = call.owner.kernel_gelu(x.reshape(-1, w.shape[1]), w, b, call.pre)
        shape = x.shape[:-1] + (w.shape[0],)
        if call.pre:
            ctx.save_for_backward(x, w, _shaped(z2, shape))
        ctx.call = call
        ctx.has_bias = b is not None
        return _shaped(y2, shape)

    @staticmethod
    def backward(ctx, g):
        x, w, z = ctx.saved_tensors
        call = ctx.call
        fused = call.owner._backward(g, z, w, gelu=True) if ctx.needs_input_grad[0] else None
        if fused is not None:
            g_z, dx = fused
        else:
            g_z = torch.ops.aten.gelu_backward(g, z, approximate="none")
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
        y = _shaped(call.owner.kernel_bare(x.reshape(-1, w.shape[1]), w, b), x.shape[:-1] + (w.shape[0],))
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
    device_type = "cuda"           # (the tests of the eligibility rules run the rules on host tensors)

    def __init__(self, ode):
        self._ode = weakref.ref(ode)
        self.plans = []            # [(sequential, {child index: (linear, tanh)})]
        self.mode = "auto"
        self.disabled = False      # the forward check failed
        self.why = None
        self.checked = False
        self.n_fused = 0           # pair calls that ran as one launch
        self._warned = False
        self._ok = {}              # (rows, out_f, in_f) -> pn_linear_fwd_supported
        # the pair's backward as one launch (pn_linear_bwd): -pn_linear_bwd auto|0|1
        self.bwd_mode = "auto"
        self.bwd_disabled = False  # the backward check failed (the forward stays fused)
        self.bwd_why = None
        self.bwd_checked = False
        self.n_fused_bwd = 0       # pair backwards that ran as one launch
        self._warned_bwd = False
        self._ok_bwd = {}          # (rows, out_f, in_f) -> pn_linear_bwd_supported
        # the bare layers (-pn_linear_bare 0|1): a map of their own; their checks switch off nothing but themselves
        self.bare = []             # [(sequential, {child index: linear})]
        self.bare_mode = "0"
        self.bare_disabled = False      # the bare forward check failed
        self.bare_why = None
        self.bare_checked = False
        self.n_bare = 0            # bare layer calls that ran pn_linear_fwd with the identity
        self.bare_bwd_disabled = False  # the bare backward check failed (the bare forward stays)
        self.bare_bwd_why = None
        self.bare_bwd_checked = False
        self.n_bare_bwd = 0        # bare backwards that ran pn_linear_dx
        self._ok_dx = {}           # (rows, out_f, in_f) -> pn_linear_dx_supported
        # the Linear -> ReLU pairs (-pn_linear_relu 0|1): a map, flags and counters of their own, as the bare layers'
        self.relu = []             # [(sequential, {child index: (linear, relu)})]
        self.relu_mode = "0"
        self.relu_disabled = False      # the ReLU forward check failed
        self.relu_why = None
        self.relu_checked = False
        self.n_relu = 0            # ReLU pair calls that ran as one launch
        self.relu_bwd_disabled = False  # the ReLU backward check failed (the ReLU forward stays)
        self.relu_bwd_why = None
        self.relu_bwd_checked = False
        self.n_relu_bwd = 0        # ReLU pair backwards that ran as one launch (pn_linear_bwd_act)
        self._warned_relu = False
        self._warned_relu_bwd = False
        # the Linear -> Sigmoid pairs (-pn_linear_sigmoid 0|1): the same in one record
        self.sig = _PairState("Sigmoid", "-pn_linear_sigmoid", "torch.sigmoid(F.linear)", "sigmoid_backward + matmul")
        # the Linear -> GELU pairs (-pn_linear_gelu 0|1): one more record; the pairs that save their pre-activation
        self.gelu = _PairState("GELU", "-pn_linear_gelu", "F.gelu(F.linear)", "gelu_backward + matmul")
        # the Linear -> Softplus and Linear -> ELU pairs (-pn_linear_softplus 0|1, -pn_linear_elu 0|1): a record each
        self.softplus, self.elu = self.kinds = _KINDS()

    def install(self, func, params, mode="auto", bwd_mode="auto", bare_mode="0", relu_mode="0", sigmoid_mode="0", gelu_mode="0",
                softplus_mode="0", elu_mode="0"):
        """Find the eligible pairs of `func` (and, with bare_mode "1", its bare layers; with relu_mode "1", its Linear -> ReLU pairs; with
        sigmoid_mode "1", its Linear -> Sigmoid pairs; with gelu_mode "1", its Linear -> GELU pairs; with softplus_mode / elu_mode "1",
        its Linear -> Softplus / Linear -> ELU pairs); returns True when there is at least one."""
        self.mode = mode
        self.bwd_mode = bwd_mode
        self.bare_mode = bare_mode
        self.relu_mode = relu_mode
        self.sig.mode = sigmoid_mode
        self.sig.refused = None
        self.gelu.mode = gelu_mode
        self.gelu.refused = None
        self.softplus.mode, self.elu.mode = softplus_mode, elu_mode
        found, refused, self.bare = find_layers(func, params, relu_mode == "1", sigmoid=sigmoid_mode == "1", gelu=gelu_mode == "1",
                                                softplus=softplus_mode == "1", elu=elu_mode == "1")
        for st in (self.gelu,) + self.kinds:
            st.static_why = next((why for key, why in refused.items() if isinstance(key, tuple) and key[1] == st.name), None)
        self.plans, self.relu, self.sig.plans, self.gelu.plans = [], [], [], []
        for st in self.kinds:
            st.plans, st.refused = [], None
        for seq, pairs in found:
            for kind, plans in ((nn.Tanh, self.plans), (nn.ReLU, self.relu), (nn.Sigmoid, self.sig.plans), (nn.GELU, self.gelu.plans)) \
                    + tuple((st.kind, st.plans) for st in self.kinds):
                mine = {i: p for i, p in pairs.items() if type(p[1]) is kind}
                if mine:
                    plans.append((seq, mine))
        if mode == "1" and refused:
            for key, why in refused.items():
                cls, name = key if isinstance(key, tuple) else (key, "Tanh")
                by_name = {st.name: st for st in (self.gelu,) + self.kinds}
                if name in by_name:
                    if by_name[name].warned:
                        continue
                elif self.sig.warned if name == "Sigmoid" else (self._warned_relu if name == "ReLU" else self._warned):
                    continue
                warnings.warn("pnode_amd: -pn_linear_fwd 1: a Linear -> %s pair of %s runs the stock modules: %s" % (name, cls, why), RuntimeWarning)
            self._warned = self._warned or any(not isinstance(key, tuple) for key in refused)
            self._warned_relu = self._warned_relu or any(isinstance(key, tuple) and key[1] == "ReLU" for key in refused)
            self.sig.warned = self.sig.warned or any(isinstance(key, tuple) and key[1] == "Sigmoid" for key in refused)
            for st in (self.gelu,) + self.kinds:
                st.warned = st.warned or any(isinstance(key, tuple) and key[1] == st.name for key in refused)
        return self.active or bool(self.plans)

    @property
    def bare_active(self):
        return self.bare_mode == "1" and bool(self.bare) and not self.bare_disabled

    @property
    def relu_active(self):
        return self.relu_mode == "1" and bool(self.relu) and not self.relu_disabled

    @property
    def active(self):
        return (bool(self.plans) and not self.disabled) or self.bare_active or self.relu_active or self.sig.active or self.gelu.active \
            or any(st.active for st in self.kinds)

    # what the Sigmoid pairs' record holds, under the names the tanh and ReLU pairs' fields have
    @property
    def sigmoid(self):
        return self.sig.plans

    @property
    def sigmoid_active(self):
        return self.sig.active

    @property
    def sigmoid_status(self):
        return self.sig.status

    @property
    def n_sigmoid(self):
        return self.sig.n

    @property
    def n_sigmoid_bwd(self):
        return self.sig.n_bwd

    # ... and the GELU pairs' (`gelu` is the record itself)
    @property
    def gelu_active(self):
        return self.gelu.active

    @property
    def gelu_status(self):
        return self.gelu.status

    @property
    def n_gelu(self):
        return self.gelu.n

    @property
    def n_gelu_bwd(self):
        return self.gelu.n_bwd

    # ... and the Softplus and ELU pairs' (`softplus` and `elu` are the records themselves)
    @property
    def softplus_status(self):
        return self.softplus.status

    @property
    def elu_status(self):
        return self.elu.status

    def _state(self, act):
        """The record of `act`'s kind where the kind is told by its record alone (Softplus, ELU), else None."""
        return next((st for st in self.kinds if type(act) is st.kind), None)

    # the one place the device is touched: tests of the eligibility rules replace it by the torch expression
    def kernel(self, x2, w, b):
        return self._ode()._ops.linear_fwd(x2, w, b, True)

    def kernel_bare(self, x2, w, b):
        return self._ode()._ops.linear_fwd(x2, w, b, False)

    def kernel_relu(self, x2, w, b):
        return self._ode()._ops.linear_fwd(x2, w, b, False, act="relu")

    def kernel_sigmoid(self, x2, w, b):
        return self._ode()._ops.linear_fwd(x2, w, b, False, act="sigmoid")

    def kernel_act(self, act, x2, w, b):
        """The saved-output pairs named by `act` ("softplus", "elu")."""
        return self._ode()._ops.linear_fwd(x2, w, b, False, act=act)

    def kernel_gelu(self, x2, w, b, pre):
        """(y, z): z the pre-activation from the same launch (pn_linear_fwd_pre) when `pre`, else None and no tensor allocated for it."""
        ops = self._ode()._ops
        if not pre:
            return ops.linear_act_fwd(x2, w, b, "gelu"), None
        z = torch.empty((x2.shape[0], w.shape[0]), dtype=x2.dtype, device=x2.device)
        return ops.linear_act_fwd(x2, w, b, "gelu", z=z), z

    def supported(self, rows, out_f, in_f):
        key = (rows, out_f, in_f)
        ok = self._ok.get(key)
        if ok is None:
            ops = self._ode()._ops
            ok = self._ok[key] = bool(hasattr(ops, "linear_fwd_supported") and ops.linear_fwd_supported(rows, out_f, in_f))
        return ok

    def _refuse(self, why, relu=False, sigmoid=False, gelu=False, st=None):
        st = self.gelu if gelu else st
        if st is not None:
            if self.mode == "1" and not st.warned:
                st.warned = True
                warnings.warn("pnode_amd: -pn_linear_fwd 1: a Linear -> %s pair runs the stock modules: %s" % (st.name, why), RuntimeWarning)
            return None
        if self.mode == "1" and not (self.sig.warned if sigmoid else (self._warned_relu if relu else self._warned)):
            if sigmoid:
                self.sig.warned = True
            elif relu:
                self._warned_relu = True
            else:
                self._warned = True
            warnings.warn("pnode_amd: -pn_linear_fwd 1: a Linear -> %s pair runs the stock modules: %s"
                          % ("Sigmoid" if sigmoid else ("ReLU" if relu else "Tanh"), why), RuntimeWarning)
        return None

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

    def _check_sigmoid(self, x, w, b, a):
        """First fused call of a Sigmoid pair of a solver: against torch.sigmoid(F.linear), |y - ref| <= CHECK_TOL (sum |x w| + |b|) +
        4 * 2^-24.  The absolute term: sigma maps a zero pre-activation to 0.5 with a rounding of its own on either side (the kernel at
        most 2.5 ulp of 2^-24, the library about 1), where tanh and ReLU give an exact 0 -- a small sum |x w| + |b| is no miss.  A miss
        switches off the Sigmoid pairs only."""
        st = self.sig
        st.checked = True
        with torch.no_grad():
            x2 = x.reshape(-1, w.shape[1])
            ref = torch.sigmoid(F.linear(x2, w, b))
            scale = x2.abs() @ w.abs().t()
            if b is not None:
                scale = scale + b.abs()
            ok = torch.isfinite(ref) & torch.isfinite(scale)
            if not bool(ok.any()):
                st.checked = False
                return True
            bar = CHECK_TOL * scale + 4.0 * 2.0 ** -24
            over = ((a.reshape(ref.shape) - ref).abs() / bar)[ok].max()
        if not float(over) <= 1.0:
            st.disabled = True
            st.why = "pn_linear_fwd and %s differ by %.2f times the bar %.0e (sum |x w| + |b|) + 4 * 2^-24" % (st.torch_fwd, float(over), CHECK_TOL)
            warnings.warn("pnode_amd: the fused Linear -> %s forward is switched off for this solver: %s" % (st.name, st.why), RuntimeWarning)
            return False
        return True

    def _check_state(self, st, x, w, b, a):
        """First fused call of a Softplus or ELU pair of a solver: against st.fwd(F.linear) at the Sigmoid pairs' bar, |y - ref| <=
        CHECK_TOL (sum |x w| + |b|) + 4 * 2^-24.  The absolute term: Softplus maps a zero pre-activation to log 2, with a rounding of
        its own on either side; ELU's rows of scale 0 are an exact 0 and need a bar above 0.  A miss switches off that kind only."""
        st.checked = True
        with torch.no_grad():
            x2 = x.reshape(-1, w.shape[1])
            ref = st.fwd(F.linear(x2, w, b))
            scale = x2.abs() @ w.abs().t()
            if b is not None:
                scale = scale + b.abs()
            ok = torch.isfinite(ref) & torch.isfinite(scale)
            if not bool(ok.any()):
                st.checked = False
                return True
            bar = CHECK_TOL * scale + 4.0 * 2.0 ** -24
            over = ((a.reshape(ref.shape) - ref).abs() / bar)[ok].max()
        if not float(over) <= 1.0:
            st.disabled = True
            st.why = "pn_linear_fwd and %s differ by %.2f times the bar %.0e (sum |x w| + |b|) + 4 * 2^-24" % (st.torch_fwd, float(over), CHECK_TOL)
            warnings.warn("pnode_amd: the fused Linear -> %s forward is switched off for this solver: %s" % (st.name, st.why), RuntimeWarning)
            return False
        return True

    def _check_gelu(self, x, w, b, a, z=None):
        """First fused call of a GELU pair of a solver: against F.gelu(F.linear), |y - ref| <= CHECK_TOL (sum |x w| + |b|) + 4 * 2^-24.
        The absolute term: GELU crosses zero at z = 0 -- a row with x = 0 and b = 0 has the scale 0 and the bar must stay above it; next
        to it the two erff (the kernel's and the library's) differ by their own ulps of a value up to 1, not of y.  z, where the call
        wrote it: against F.linear in the bare layer's measure.  A miss switches off the GELU pairs only."""
        st = self.gelu
        st.checked = True
        with torch.no_grad():
            x2 = x.reshape(-1, w.shape[1])
            lin = F.linear(x2, w, b)
            ref = F.gelu(lin)
            scale = x2.abs() @ w.abs().t()
            if b is not None:
                scale = scale + b.abs()
            ok = torch.isfinite(ref) & torch.isfinite(scale)
            if not bool(ok.any()):
                st.checked = False
                return True
            bar = CHECK_TOL * scale + 4.0 * 2.0 ** -24
            over = ((a.reshape(ref.shape) - ref).abs() / bar)[ok].max()
            what = "pn_linear_fwd and %s" % st.torch_fwd
            if z is not None and float(over) <= 1.0:
                over = ((z.reshape(ref.shape) - lin).abs() / bar)[ok].max()
                what = "the pre-activation of pn_linear_fwd_pre and F.linear"
        if not float(over) <= 1.0:
            st.disabled = True
            st.why = "%s differ by %.2f times the bar %.0e (sum |x w| + |b|) + 4 * 2^-24" % (what, float(over), CHECK_TOL)
            warnings.warn("pnode_amd: the fused Linear -> %s forward is switched off for this solver: %s" % (st.name, st.why), RuntimeWarning)
            return False
        return True

    def _check(self, x, w, b, a, bare=False, relu=False):
        """First fused call of a solver: the pair through torch as well.  bare: a bare layer's first call, against F.linear in the same
        measure; a miss switches off the bare path only.  relu: a ReLU pair's first call, against torch.relu(F.linear) in the same
        measure (ReLU is 1-Lipschitz: the bare layer's bar carries over); a miss switches off the ReLU pairs only."""
        done = "bare_checked" if bare else ("relu_checked" if relu else "checked")
        setattr(self, done, True)
        with torch.no_grad():
            x2 = x.reshape(-1, w.shape[1])
            ref = F.linear(x2, w, b)
            if relu:
                ref = torch.relu(ref)
            elif not bare:
                ref = torch.tanh(ref)
            scale = x2.abs() @ w.abs().t()
            if b is not None:
                scale = scale + b.abs()
            ok = torch.isfinite(ref) & (scale > 0)
            if not bool(ok.any()):
                setattr(self, done, False)
                return True
            err = float(((a.reshape(ref.shape) - ref).abs() / scale)[ok].max())
        if not err <= CHECK_TOL:
            if bare:
                self.bare_disabled = True
                self.bare_why = "pn_linear_fwd and F.linear differ by %.2e of sum |x w| + |b| (allowed: %.0e)" % (err, CHECK_TOL)
                warnings.warn("pnode_amd: the bare Linear layers run the stock modules for this solver: " + self.bare_why, RuntimeWarning)
                return False
            if relu:
                self.relu_disabled = True
                self.relu_why = "pn_linear_fwd and torch.relu(F.linear) differ by %.2e of sum |x w| + |b| (allowed: %.0e)" % (err, CHECK_TOL)
                warnings.warn("pnode_amd: the fused Linear -> ReLU forward is switched off for this solver: " + self.relu_why, RuntimeWarning)
                return False
            self.disabled = True
            self.why = "pn_linear_fwd and torch.tanh(F.linear) differ by %.2e of sum |x w| + |b| (allowed: %.0e)" % (err, CHECK_TOL)
            warnings.warn("pnode_amd: the fused Linear -> Tanh forward is switched off for this solver: " + self.why, RuntimeWarning)
            return False
        return True

    # ---- the backward of a pair (called from _LinearTanh.backward)
    def kernel_bwd(self, g2, a2, w):
        return self._ode()._ops.linear_bwd(g2, a2, w)

    def supported_bwd(self, rows, out_f, in_f, entry="linear_bwd"):
        key = (rows, out_f, in_f)
        cache = self._ok_bwd if entry == "linear_bwd" else self._ok_dx
        ok = cache.get(key)
        if ok is None:
            ops = self._ode()._ops
            ok = cache[key] = bool(hasattr(ops, entry + "_supported") and getattr(ops, entry + "_supported")(rows, out_f, in_f))
        return ok

    def kernel_bwd_relu(self, g2, a2, w):
        return self._ode()._ops.linear_bwd(g2, a2, w, act="relu")

    def kernel_bwd_sigmoid(self, g2, a2, w):
        return self._ode()._ops.linear_bwd(g2, a2, w, act="sigmoid")

    def kernel_bwd_act(self, act, g2, a2, w):
        return self._ode()._ops.linear_bwd(g2, a2, w, act=act)

    def kernel_bwd_gelu(self, g2, z2, w):
        return self._ode()._ops.linear_bwd(g2, z2, w, act="gelu")

    def _bwd_fusable(self, g, a, w, relu=False, sigmoid=False, gelu=False, st=None):
        """None, or the reason (a string) this backward runs the torch operations.  a: the pair's output; None for a bare layer
        (pn_linear_dx: the same rules minus everything about a).  relu: a ReLU pair (pn_linear_bwd_act: the rules of a tanh pair, and
        a backend with `linear_relu`).  sigmoid: a Sigmoid pair (the same, and a backend with `linear_sigmoid`).  gelu: a GELU pair (the same, and a
        backend with `linear_gelu`; `a` is then the pair's pre-activation).  st: a Softplus or ELU pair's record (the same, and a backend with
        `linear_softplus` / `linear_elu`)."""
        bare = a is None
        entry = "linear_dx" if bare else "linear_bwd"
        ode = self._ode()
        if ode is None or not hasattr(ode._ops, entry):
            return "the backend has no " + entry
        if relu and not getattr(ode._ops, "linear_relu", False):
            return "the backend has no linear_relu"
        if sigmoid and not getattr(ode._ops, "linear_sigmoid", False):
            return "the backend has no linear_sigmoid"
        if gelu and not getattr(ode._ops, "linear_gelu", False):
            return "the backend has no linear_gelu"
        if st is not None and not getattr(ode._ops, "linear_" + st.act, False):
            return "the backend has no linear_" + st.act
        if self.bwd_mode == "0":
            return "-pn_linear_bwd 0"
        if st is not None:
            if st.bwd_disabled:
                return st.bwd_why
        elif gelu:
            if self.gelu.bwd_disabled:
                return self.gelu.bwd_why
        elif sigmoid:
            if self.sig.bwd_disabled:
                return self.sig.bwd_why
        elif relu:
            if self.relu_bwd_disabled:
                return self.relu_bwd_why
        elif self.bare_bwd_disabled if bare else self.bwd_disabled:
            return self.bare_bwd_why if bare else self.bwd_why
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != w.device or g.device.type != self.device_type \
                or (g.dim() < 1 or g.shape[-1] != w.shape[0] if bare else g.shape != a.shape):
            return "the cotangent is no fp32 tensor of the pair's shape on the weight's device"
        if not (g.is_contiguous() and (bare or a.is_contiguous()) and w.is_contiguous()):
            return "the cotangent is not contiguous"
        if g.data_ptr() % 16 or (not bare and a.data_ptr() % 16) or w.data_ptr() % 16:
            return "operands are not 16-byte aligned"
        if _autocast_on(g.device.type):
            return "autocast is on"
        if torch.is_grad_enabled():
            return "the backward pass is itself differentiated (create_graph)"
        if not self.supported_bwd(g.numel() // w.shape[0], w.shape[0], w.shape[1], entry):
            return "outside pn_%s_supported" % entry
        return None

    def _check_bwd(self, g2, a2, w, gz, dx):
        """First fused backward of a solver: both results through torch as well.  gz to 3 * 2^-24 |g| (two roundings in 1 - a^2, one in
        the product, with or without an fma), dx to CHECK_TOL of |gz| |w| (the forward's bar in the forward's measure).  Returns None, or
        the torch results after switching the fused backward -- only it -- off."""
        self.bwd_checked = True
        gz_t = torch.ops.aten.tanh_backward(g2, a2)
        dx_t = torch.matmul(gz_t, w)
        scale = gz_t.abs() @ w.abs()
        fin = torch.isfinite(gz_t)
        ok = torch.isfinite(dx_t) & (scale > 0)
        if not bool(fin.any()) or not bool(ok.any()):
            self.bwd_checked = False               # nothing to judge by: the next call is checked
            return None
        bad_z = bool((~((gz - gz_t).abs() <= 3.0 * 2.0 ** -24 * g2.abs()) & fin).any())
        err = float(((dx - dx_t).abs() / scale)[ok].max())
        if bad_z or not err <= CHECK_TOL:
            self.bwd_disabled = True
            self.bwd_why = "pn_linear_bwd and tanh_backward + matmul differ: " + (
                "g_z by more than 3 * 2^-24 |g|" if bad_z else "dx by %.2e of |g_z| |w| (allowed: %.0e)" % (err, CHECK_TOL))
            warnings.warn("pnode_amd: the fused Linear -> Tanh backward is switched off for this solver: " + self.bwd_why, RuntimeWarning)
            return gz_t, dx_t
        return None

    def _check_relu_bwd(self, g2, a2, w, gz, dx):
        """First fused backward of a ReLU pair of a solver: both results through torch as well.  gz has no arithmetic in it: it must be
        threshold_backward's bit for bit; dx to CHECK_TOL of |gz| |w| (the tanh pair's bar in its measure).  Returns None, or the torch
        results after switching the fused ReLU backward -- only it -- off."""
        self.relu_bwd_checked = True
        gz_t = torch.ops.aten.threshold_backward(g2, a2, 0)
        dx_t = torch.matmul(gz_t, w)
        scale = gz_t.abs() @ w.abs()
        ok = torch.isfinite(dx_t) & (scale > 0)
        bad_z = not torch.equal(gz.view(torch.int32), gz_t.view(torch.int32))
        if not bad_z and not bool(ok.any()):
            self.relu_bwd_checked = False          # nothing to judge dx by: the next call is checked
            return None
        err = float(((dx - dx_t).abs() / scale)[ok].max()) if bool(ok.any()) else 0.0
        if bad_z or not err <= CHECK_TOL:
            self.relu_bwd_disabled = True
            self.relu_bwd_why = "pn_linear_bwd_act and threshold_backward + matmul differ: " + (
                "g_z is not threshold_backward's bit for bit" if bad_z else "dx by %.2e of |g_z| |w| (allowed: %.0e)" % (err, CHECK_TOL))
            warnings.warn("pnode_amd: the fused Linear -> ReLU backward is switched off for this solver: " + self.relu_bwd_why, RuntimeWarning)
            return gz_t, dx_t
        return None

    def _check_sigmoid_bwd(self, g2, a2, w, gz, dx):
        """First fused backward of a Sigmoid pair of a solver: both results through torch as well.  gz to 1.5 * 2^-24 |g| of
        sigmoid_backward's, elementwise (two roundings here, three there, each relative to |g a (1 - a)| <= |g| / 4); dx to CHECK_TOL of
        |gz| |w| (the pairs' measure).  Returns None, or the torch results after switching the fused Sigmoid backward -- only it -- off."""
        st = self.sig
        st.bwd_checked = True
        gz_t = torch.ops.aten.sigmoid_backward(g2, a2)
        dx_t = torch.matmul(gz_t, w)
        scale = gz_t.abs() @ w.abs()
        fin = torch.isfinite(gz_t)
        ok = torch.isfinite(dx_t) & (scale > 0)
        if not bool(fin.any()) or not bool(ok.any()):
            st.bwd_checked = False                 # nothing to judge by: the next call is checked
            return None
        bad_z = bool((~((gz - gz_t).abs() <= 1.5 * 2.0 ** -24 * g2.abs()) & fin).any())
        err = float(((dx - dx_t).abs() / scale)[ok].max())
        if bad_z or not err <= CHECK_TOL:
            st.bwd_disabled = True
            st.bwd_why = "pn_linear_bwd_act and %s differ: " % st.torch_bwd + (
                "g_z by more than 1.5 * 2^-24 |g|" if bad_z else "dx by %.2e of |g_z| |w| (allowed: %.0e)" % (err, CHECK_TOL))
            warnings.warn("pnode_amd: the fused Linear -> %s backward is switched off for this solver: %s" % (st.name, st.bwd_why), RuntimeWarning)
            return gz_t, dx_t
        return None

    def _check_state_bwd(self, st, g2, a2, w, gz, dx):
        """First fused backward of a Softplus or ELU pair of a solver: both results through torch as well.  gz to st.gz_bar * 2^-24 |g|
        of st.gz(g, a), elementwise -- Softplus 4: either side's expm1 is held to that of the exact g (1 - e^-a) (the kernel's by its GPU
        test), and they are the same function of the same library; ELU 1.5: one rounded add, one rounded product on both sides --; dx to
        CHECK_TOL of |gz| |w| (the pairs' measure).  Returns None, or the torch results after switching that kind's fused backward --
        only it -- off."""
        st.bwd_checked = True
        gz_t = st.gz(g2, a2)
        dx_t = torch.matmul(gz_t, w)
        scale = gz_t.abs() @ w.abs()
        fin = torch.isfinite(gz_t)
        ok = torch.isfinite(dx_t) & (scale > 0)
        if not bool(fin.any()) or not bool(ok.any()):
            st.bwd_checked = False                 # nothing to judge by: the next call is checked
            return None
        bad_z = bool((~((gz - gz_t).abs() <= st.gz_bar * 2.0 ** -24 * g2.abs()) & fin).any())
        err = float(((dx - dx_t).abs() / scale)[ok].max())
        if bad_z or not err <= CHECK_TOL:
            st.bwd_disabled = True
            st.bwd_why = "pn_linear_bwd_act and %s differ: " % st.torch_bwd + (
                "g_z by more than %g * 2^-24 |g|" % st.gz_bar if bad_z else "dx by %.2e of |g_z| |w| (allowed: %.0e)" % (err, CHECK_TOL))
            warnings.warn("pnode_amd: the fused Linear -> %s backward is switched off for this solver: %s" % (st.name, st.bwd_why), RuntimeWarning)
            return gz_t, dx_t
        return None

    def _check_gelu_bwd(self, g2, z2, w, gz, dx):
        """First fused backward of a GELU pair of a solver: both results through torch as well.  gz to 32 * 2^-24 |g| of gelu_backward's,
        elementwise and ABSOLUTE in the derivative d = cdf + z pdf, which crosses zero near z = -0.7518 (a bar relative to |g d| would be 0
        there): each side evaluates erff once, within the 16 ulp OpenCL allows erf, of a value up to 1, halved in cdf -- 8 * 2^-24 a
        side; z pdf <= 0.25 adds less than one more; twice that for the two sides.  dx to CHECK_TOL of |gz| |w| (the pairs' measure).
        Returns None, or the torch results after switching the fused GELU backward -- only it -- off."""
        st = self.gelu
        st.bwd_checked = True
        gz_t = torch.ops.aten.gelu_backward(g2, z2, approximate="none")
        dx_t = torch.matmul(gz_t, w)
        scale = gz_t.abs() @ w.abs()
        fin = torch.isfinite(gz_t)
        ok = torch.isfinite(dx_t) & (scale > 0)
        if not bool(fin.any()) or not bool(ok.any()):
            st.bwd_checked = False                 # nothing to judge by: the next call is checked
            return None
        bad_z = bool((~((gz - gz_t).abs() <= 32.0 * 2.0 ** -24 * g2.abs()) & fin).any())
        err = float(((dx - dx_t).abs() / scale)[ok].max())
        if bad_z or not err <= CHECK_TOL:
            st.bwd_disabled = True
            st.bwd_why = "pn_linear_bwd_act and %s differ: " % st.torch_bwd + (
                "g_z by more than 32 * 2^-24 |g|" if bad_z else "dx by %.2e of |g_z| |w| (allowed: %.0e)" % (err, CHECK_TOL))
            warnings.warn("pnode_amd: the fused Linear -> %s backward is switched off for this solver: %s" % (st.name, st.bwd_why), RuntimeWarning)
            return gz_t, dx_t
        return None

    def _backward(self, g, a, w, relu=False, sigmoid=False, gelu=False, st=None):
        """(g_z, dx) of one pair by pn_linear_bwd (relu, sigmoid, gelu, st: pn_linear_bwd_act; gelu: `a` is the pre-activation; st: the
        record of a Softplus or ELU pair), or None: the caller runs tanh_backward (threshold_backward, sigmoid_backward, gelu_backward,
        st.gz) and matmul."""
        kind = st                                  # (a record of _KINDS, or None)
        st = kind if kind is not None else (self.gelu if gelu else self.sig)
        why = self._bwd_fusable(g, a, w, relu, sigmoid, gelu, kind)
        sigmoid = sigmoid or gelu or kind is not None      # (below: the pairs whose state is a record, `st`)
        if why is not None:
            if self.bwd_mode == "1" and not (st.warned_bwd if sigmoid else (self._warned_relu_bwd if relu else self._warned_bwd)):
                if sigmoid:
                    st.warned_bwd = True
                elif relu:
                    self._warned_relu_bwd = True
                else:
                    self._warned_bwd = True
                warnings.warn("pnode_amd: -pn_linear_bwd 1: the backward of a Linear -> %s pair runs the torch operations: %s"
                              % (st.name if sigmoid else ("ReLU" if relu else "Tanh"), why), RuntimeWarning)
            return None
        out_f, in_f = w.shape
        g2, a2 = g.reshape(-1, out_f), a.reshape(-1, out_f)
        with torch.no_grad():
            if kind is not None:
                gz, dx = self.kernel_bwd_act(kind.act, g2, a2, w)
                checked, check = st.bwd_checked, lambda *args: self._check_state_bwd(kind, *args)
            elif gelu:
                gz, dx = self.kernel_bwd_gelu(g2, a2, w)
                checked, check = st.bwd_checked, self._check_gelu_bwd
            elif sigmoid:
                gz, dx = self.kernel_bwd_sigmoid(g2, a2, w)
                checked, check = st.bwd_checked, self._check_sigmoid_bwd
            elif relu:
                gz, dx = self.kernel_bwd_relu(g2, a2, w)
                checked, check = self.relu_bwd_checked, self._check_relu_bwd
            else:
                gz, dx = self.kernel_bwd(g2, a2, w)
                checked, check = self.bwd_checked, self._check_bwd
            if not checked and not (g.is_cuda and torch.cuda.is_current_stream_capturing()):
                torch_way = check(g2, a2, w, gz, dx)
                if torch_way is not None:
                    gz, dx = torch_way
                    return gz.view(g.shape), dx.view(g.shape[:-1] + (in_f,))
        if sigmoid:
            st.n_bwd += 1
        elif relu:
            self.n_relu_bwd += 1
        else:
            self.n_fused_bwd += 1
        return gz.view(g.shape), dx.view(g.shape[:-1] + (in_f,))

    # ---- the backward of a bare layer (called from _Linear.backward)
    def kernel_dx(self, g2, w):
        return self._ode()._ops.linear_dx(g2, w)

    def _check_bare_bwd(self, g2, w, dx):
        """First pn_linear_dx of a solver: through torch as well, to CHECK_TOL of |g| |w| (the pair's bar in the pair's measure).  Returns
        None, or the torch result after switching the bare backward -- only it -- off."""
        self.bare_bwd_checked = True
        dx_t = torch.matmul(g2, w)
        scale = g2.abs() @ w.abs()
        ok = torch.isfinite(dx_t) & (scale > 0)
        if not bool(ok.any()):
            self.bare_bwd_checked = False          # nothing to judge by: the next call is checked
            return None
        err = float(((dx - dx_t).abs() / scale)[ok].max())
        if not err <= CHECK_TOL:
            self.bare_bwd_disabled = True
            self.bare_bwd_why = "pn_linear_dx and matmul differ: dx by %.2e of |g| |w| (allowed: %.0e)" % (err, CHECK_TOL)
            warnings.warn("pnode_amd: the backward of the bare Linear layers runs matmul for this solver: " + self.bare_bwd_why, RuntimeWarning)
            return dx_t
        return None

    def _backward_bare(self, g, w):
        """dx of one bare layer by pn_linear_dx, or None: the caller runs matmul."""
        if self._bwd_fusable(g, None, w) is not None:
            return None
        out_f, in_f = w.shape
        g2 = g.reshape(-1, out_f)
        with torch.no_grad():
            dx = self.kernel_dx(g2, w)
            if not self.bare_bwd_checked and not (g.is_cuda and torch.cuda.is_current_stream_capturing()):
                torch_way = self._check_bare_bwd(g2, w, dx)
                if torch_way is not None:
                    return torch_way.view(g.shape[:-1] + (in_f,))
        self.n_bare_bwd += 1
        return dx.view(g.shape[:-1] + (in_f,))

    @property
    def bare_status(self):
        if self.bare_mode != "1":
            return "off (-pn_linear_bare 0)"
        if not self.bare:
            return "stock modules (no eligible bare layer)"
        if self.bare_disabled:
            return "stock modules (%s)" % self.bare_why
        return "fused (%d layers; %d forward, %d backward calls so far)" % (sum(len(b) for _, b in self.bare), self.n_bare, self.n_bare_bwd)

    @property
    def relu_status(self):
        if self.relu_mode != "1":
            return "off (-pn_linear_relu 0)"
        if not self.relu:
            return "stock modules (no eligible Linear -> ReLU pair)"
        if self.relu_disabled:
            return "stock modules (%s)" % self.relu_why
        return "fused (%d pairs; %d forward, %d backward calls so far)" % (sum(len(p) for _, p in self.relu), self.n_relu, self.n_relu_bwd)

    @property
    def bwd_status(self):
        if self.bwd_mode == "0":
            return "torch operations (-pn_linear_bwd 0)"
        ode = self._ode()
        if ode is None or not hasattr(ode._ops, "linear_bwd"):
            return "torch operations (the backend has no linear_bwd)"
        if self.bwd_disabled:
            return "torch operations (%s)" % self.bwd_why
        return "fused (%d calls so far)" % self.n_fused_bwd

    def _pair(self, lin, act, x, grads):
        """One pair: Linear -> Tanh or, where `act` is an nn.ReLU, Linear -> ReLU (its module is not called: either `inplace` will do), or,
        where it is an nn.Sigmoid, Linear -> Sigmoid, an nn.GELU, Linear -> GELU, an nn.Softplus or nn.ELU, that pair (its record: `st`)."""
        relu, sigmoid, gelu = type(act) is nn.ReLU, type(act) is nn.Sigmoid, type(act) is nn.GELU
        st = self._state(act)
        why = self._fusable(lin, x)
        if why is not None:
            if sigmoid:
                self.sig.refused = why
            if gelu:
                self.gelu.refused = why
            if st is not None:
                st.refused = why
            self._refuse(why, relu, sigmoid, gelu, st)
            return act(lin(x))
        w, b = lin.weight, lin.bias
        ev = grads.recording if grads is not None else None
        if ev is not None and not grads.note_fused(lin, x):
            ev = None                             # (the evaluation is left to autograd: LinearParamGrads.end mutes it)
        call = _Call()
        call.owner, call.module, call.grads, call.ev, call.version, call.relu, call.sigmoid = self, lin, grads, ev, x._version, relu, sigmoid
        call.state = st
        if gelu:
            # the saved-pre-activation form only where somebody will differentiate the call: else y alone, and no z is allocated
            call.pre = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad))
            a = _LinearGelu.apply(x, w, b, call)
        else:
            a = _LinearTanh.apply(x, w, b, call)
        checked = self.gelu.checked if gelu else (self.sig.checked if sigmoid else (self.relu_checked if relu else self.checked))
        if st is not None:
            checked = st.checked
        if not checked and not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            args = (x.detach(), w.detach(), None if b is None else b.detach(), a.detach())
            if st is not None:
                good = self._check_state(st, *args)
            elif gelu:
                z = a.grad_fn.saved_tensors[2] if call.pre and a.grad_fn is not None else None
                good = self._check_gelu(*args, z=z)
            else:
                good = self._check_sigmoid(*args) if sigmoid else self._check(*args, relu=relu)
            if not good:
                return act(lin(x))
        if ev is not None and a.grad_fn is not None:
            ev.through[a.grad_fn] = x.grad_fn     # Evaluation.clean passes the pair along its input edge only
        if st is not None:
            st.n += 1
        elif gelu:
            self.gelu.n += 1
            self.gelu.n_pre += 1 if call.pre else 0
        elif sigmoid:
            self.sig.n += 1
        elif relu:
            self.n_relu += 1
        else:
            self.n_fused += 1
        return a

    def _bare(self, lin, x, grads):
        """One bare layer (-pn_linear_bare 1): _pair without the activation."""
        if self._fusable(lin, x) is not None:
            return lin(x)
        w, b = lin.weight, lin.bias
        ev = grads.recording if grads is not None else None
        if ev is not None and not grads.note_fused(lin, x):
            ev = None                             # (the evaluation is left to autograd: LinearParamGrads.end mutes it)
        call = _Call()
        call.owner, call.module, call.grads, call.ev, call.version, call.state = self, lin, grads, ev, x._version, None
        y = _Linear.apply(x, w, b, call)
        if not self.bare_checked and not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            if not self._check(x.detach(), w.detach(), None if b is None else b.detach(), y.detach(), bare=True):
                return lin(x)
        if ev is not None and y.grad_fn is not None:
            ev.through[y.grad_fn] = x.grad_fn     # Evaluation.clean passes the layer along its input edge only
        self.n_bare += 1
        return y

    def _off(self, act):
        """The forward check of the pairs of `act`'s kind failed."""
        if type(act) is nn.Sigmoid:
            return self.sig.disabled
        if type(act) is nn.GELU:
            return self.gelu.disabled
        if self._state(act) is not None:
            return self._state(act).disabled
        return self.relu_disabled if type(act) is nn.ReLU else self.disabled

    def _runner(self, seq, pairs, alone, grads):
        def forward(inp):
            kids = list(seq._modules.values())
            i, n = 0, len(kids)
            while i < n:
                p = pairs.get(i)
                if p is not None and i + 1 < n and kids[i] is p[0] and kids[i + 1] is p[1] \
                        and not self._off(p[1]):
                    inp = self._pair(p[0], p[1], inp, grads)
                    i += 2
                elif alone.get(i) is kids[i] and not self.bare_disabled:
                    inp = self._bare(kids[i], inp, grads)
                    i += 1
                else:
                    inp = kids[i](inp)
                    i += 1
            return inp
        return forward

    def _containers(self):
        """[(sequential, its pairs, its bare layers)]: the pairs while their forward is on (the ReLU pairs with -pn_linear_relu 1, the
        Sigmoid pairs with -pn_linear_sigmoid 1, the GELU pairs with -pn_linear_gelu 1, the Softplus and ELU pairs with their options), the
        bare layers with -pn_linear_bare 1."""
        out = {}
        if not self.disabled:
            for seq, pairs in self.plans:
                out[id(seq)] = (seq, pairs, {})
        for plans in ((self.relu,) if self.relu_active else ()) + ((self.sig.plans,) if self.sig.active else ()) \
                + ((self.gelu.plans,) if self.gelu.active else ()) + tuple(st.plans for st in self.kinds if st.active):
            for seq, pairs in plans:
                both = dict(out[id(seq)][1]) if id(seq) in out else {}      # (a copy: the container's tanh pairs stay their own map)
                both.update(pairs)
                out[id(seq)] = (seq, both, {})
        if self.bare_active:
            for seq, alone in self.bare:
                out[id(seq)] = (seq, out[id(seq)][1] if id(seq) in out else {}, alone)
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
                    if _user_hooked(seq) or any(_user_hooked(m) for pr in pairs.values() for m in pr):
                        for relu, sigmoid, gelu in sorted({(type(pr[1]) is nn.ReLU, type(pr[1]) is nn.Sigmoid, type(pr[1]) is nn.GELU)
                                                           for pr in pairs.values() if self._state(pr[1]) is None}):
                            self._refuse("a forward, pre-forward or backward hook on the pair or its container", relu, sigmoid, gelu)
                        for st in self.kinds:
                            if any(type(pr[1]) is st.kind for pr in pairs.values()):
                                self._refuse("a forward, pre-forward or backward hook on the pair or its container", st=st)
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
