"""Options database: the stand-in for ``petsc4py.init(sys.argv)`` + ``ts.setFromOptions()``.

The reference's drivers pass every argv token argparse does not know to PETSc
(``examples-pnode/ode_demo_petsc.py:46,63-66``) and ``ODEPetsc.setupTS`` ends with
``self.ts.setFromOptions()`` (``pnode/petsc_adjoint.py:775``), so PETSc command-line options
override the ``method`` keyword, the controller, tolerances and the checkpointing mode.  The
same spellings are honoured here: call ``pnode_amd.init(sys.argv)`` where the reference calls
``petsc4py.init(sys.argv)``; options can also come from the ``PETSC_OPTIONS`` environment
variable (PETSc reads it too) or ``set_option``.

The engine's own options (``-pn_*``, no PETSc spelling) are read from the same database where they act; README.md lists
them.  ``-pn_linear_fwd auto|0|1`` (pnode_amd/_linearfwd.py, read in ``RKSweep._setup_linear_fwd``): ``auto``, the default, runs the
eligible ``nn.Linear -> nn.Tanh`` pairs of func as one ``pn_linear_fwd`` launch each inside the solver's own evaluations; ``0`` runs
the stock modules everywhere; ``1`` is ``auto`` and warns once, with the reason, about a pair that cannot be fused.
``-pn_linear_bwd auto|0|1`` (read in the same place): ``auto``, the default, runs the backward of such a pair -- ``g_z = g (1 - a^2)``
and ``dx = g_z W`` -- as one ``pn_linear_bwd`` launch; ``0`` runs ``tanh_backward`` and ``matmul`` by torch; ``1`` is ``auto`` and
warns once with the reason a pair's backward runs through torch.  It has no effect where ``-pn_linear_fwd`` leaves the stock modules
in place: the backward lives in the pair's ``autograd.Function``.
``-pn_linear_form auto|plain`` (read there too): ``auto``, the default, lets ``pn_linear_fwd`` and ``pn_linear_bwd`` take the pipelined
K loop on aligned shapes; ``plain`` keeps the plain loop everywhere (``PN_LINEAR_FORM_PLAIN``).  The two give the same bits: the option
is for timing one against the other inside one tree.
``-pn_linear_bare 0|1`` (read there too): ``0``, the default, leaves func's bare ``nn.Linear`` layers -- no ``nn.Tanh`` behind them: the
head of every ``... -> Linear`` net -- to the stock module; ``1`` runs the eligible ones through ``pn_linear_fwd`` with the identity and
their backward ``dx = g W`` through ``pn_linear_dx`` (``-pn_linear_bwd 0`` keeps ``matmul``), inside the solver's own evaluations, under
the rules of the pairs.  ``ode.linear_bare`` reports what runs.  ``-pn_linear_fwd 0`` switches this off with the pairs.
``-pn_linear_relu 0|1`` (read there too; anything else is refused): ``0``, the default, leaves a Linear in front of an ``nn.ReLU`` what it
is -- a stock module, or a bare layer under ``-pn_linear_bare 1``; ``1`` runs the eligible ``nn.Linear -> nn.ReLU`` pairs as one
``pn_linear_fwd`` launch with ``PN_ACT_RELU`` and their backward -- ``g_z = threshold_backward(g, a, 0)``, ``dx = g_z W`` -- as one
``pn_linear_bwd_act`` launch (``-pn_linear_bwd 0`` keeps ``threshold_backward`` and ``matmul``), under the rules of the Tanh pairs.
``ode.linear_relu`` reports what runs.  ``-pn_linear_fwd 0`` switches this off too.
``-pn_linear_sigmoid 0|1`` (read there too; anything else is refused): the same for the ``nn.Linear -> nn.Sigmoid`` pairs (exactly those
types): ``0``, the default, leaves such a Linear a stock module, or a bare layer under ``-pn_linear_bare 1``; ``1`` runs the pair as one
``pn_linear_fwd`` launch with ``PN_ACT_SIGMOID`` (``1 / (1 + expf(-z))``, within 2.5 * 2^-24 of sigma: not ``torch.sigmoid``'s bits) and
its backward -- ``g_z = g a (1 - a)``, ``dx = g_z W`` -- as one ``pn_linear_bwd_act`` launch (``-pn_linear_bwd 0`` keeps
``sigmoid_backward`` and ``matmul``).  ``ode.linear_sigmoid`` reports what runs.  ``-pn_linear_fwd 0`` switches this off too.
``-pn_linear_gelu 0|1`` (read there too; anything else is refused): the same for the ``nn.Linear -> nn.GELU`` pairs (exactly those types,
``approximate='none'``): ``0``, the default, leaves such a Linear a stock module, or a bare layer under ``-pn_linear_bare 1``; ``1`` runs
the pair as one launch that writes the pre-activation ``z`` beside ``y`` where the evaluation will be differentiated
(``pn_linear_fwd_pre``; ``z`` is what the pair saves) and ``y`` alone elsewhere (``pn_linear_fwd`` with ``PN_ACT_GELU``), and its backward
-- ``g_z = g (cdf + z pdf)``, ``dx = g_z W`` -- as one ``pn_linear_bwd_act`` launch reading ``z`` (``-pn_linear_bwd 0`` keeps
``gelu_backward`` and ``matmul``).  ``ode.linear_gelu`` reports what runs.  ``-pn_linear_fwd 0`` switches this off too.
``-pn_linear_softplus 0|1``, ``-pn_linear_elu 0|1`` (read there too; anything else is refused): the same for the ``nn.Linear -> nn.Softplus`` (``beta == 1``, ``threshold == 20``) and ``nn.Linear -> nn.ELU`` (``alpha == 1``) pairs, saved-output pairs as the Sigmoid ones (``PN_ACT_SOFTPLUS``, ``PN_ACT_ELU``; ``ode.linear_softplus``, ``ode.linear_elu``).
"""
import os
import shlex

_DB = {}


def _is_key(tok):
    if not tok.startswith("-") or len(tok) < 2:
        return False
    try:
        float(tok)
        return False          # a negative number is a value, not a key
    except ValueError:
        return True


def parse(argv):
    """['-ts_adapt_type', 'none', '-ts_monitor'] -> {'ts_adapt_type': 'none', 'ts_monitor': ''}"""
    out = {}
    toks = list(argv)
    i = 0
    while i < len(toks):
        tok = toks[i]
        if _is_key(tok):
            key = tok.lstrip("-")
            if i + 1 < len(toks) and not _is_key(toks[i + 1]):
                out[key] = str(toks[i + 1])
                i += 2
            else:
                out[key] = ""
                i += 1
        else:
            i += 1
    return out


def init(argv=None):
    """Fill the database from PETSC_OPTIONS and `argv` (argv[0] is skipped like PETSc does)."""
    _DB.clear()
    env = os.environ.get("PETSC_OPTIONS")
    if env:
        _DB.update(parse(shlex.split(env)))
    if argv:
        _DB.update(parse(list(argv)[1:]))
    return dict(_DB)


def set_option(key, value=""):
    _DB[key.lstrip("-")] = "" if value is None else str(value)


def del_option(key):
    _DB.pop(key.lstrip("-"), None)


def clear():
    _DB.clear()


def get_all():
    return dict(_DB)


def truthy(value, default=True):
    """PETSc bool parsing: a bare flag means true."""
    if value is None:
        return default
    v = str(value).strip().lower()
    if v == "":
        return True
    return v in ("1", "true", "yes", "on")


def linear_form():
    """-pn_linear_form auto|plain; anything else is refused by name."""
    v = str(_DB.get("pn_linear_form", "auto")).strip().lower()
    if v not in ("auto", "plain"):
        raise ValueError("-pn_linear_form %r: auto or plain" % v)
    return v
