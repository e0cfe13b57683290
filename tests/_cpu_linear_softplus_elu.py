"""TEST SCAFFOLDING -- the CPU stand-in of tests/_cpu_linear_gelu.py with the Softplus and ELU acts: ``pn_linear_fwd`` with
``PN_ACT_SOFTPLUS`` / ``PN_ACT_ELU`` and ``pn_linear_bwd_act`` are stood in for by the four formulas of the kernels, spelled in torch --
``z > 20 ? z : log1p(exp(z))``, ``z > 0 ? z : expm1(z)``, ``g * (-expm1(-a))``, ``a > 0 ? g : g * (a + 1)`` -- and every call is counted
by name (``fwd_softplus``, ``bwd_elu``, ...)."""
import torch
import torch.nn.functional as F

from _cpu_linear_gelu import ACT, GeluOps, NoGeluOps


def softplus_y(z):
    return torch.where(z > 20.0, z, torch.log1p(torch.exp(z)))


def elu_y(z):
    return torch.where(z > 0.0, z, torch.expm1(z))


def softplus_gz(g, a):
    return g * (-torch.expm1(-a))


def elu_gz(g, a):
    return torch.where(a > 0.0, g, g * (a + 1.0))


FWD = dict(ACT, softplus=softplus_y, elu=elu_y)
GZ = {"softplus": softplus_gz, "elu": elu_gz}


class NoSoftplusEluOps(GeluOps):
    """Every entry point and every older capability, but neither `linear_softplus` nor `linear_elu`: the forward takes the names (it asks
    for no capability, as the Sigmoid pairs'), the backward is refused by the engine."""
    def linear_act_fwd(self, x, w, b, act, y=None, z=None, flags=None):
        if act not in GZ:
            return super().linear_act_fwd(x, w, b, act, y=y, z=z, flags=flags)
        assert self.linear_fwd_supported(x.shape[0], w.shape[0], w.shape[1]) and x.dim() == 2 and x.is_contiguous()
        self.count("fwd_" + act + ("" if z is None else "_pre"))
        lin = F.linear(x, w, b)
        if z is not None:
            z.copy_(lin)
        return FWD[act](lin)

    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        if act not in GZ:
            return super().linear_bwd(g, a, w, gz=gz, dx=dx, flags=flags, act=act)
        assert g.dim() == 2 and g.is_contiguous() and a.shape == g.shape
        self.count("bwd_" + act)
        gz = GZ[act](g, a)
        return gz, torch.matmul(gz, w)


class SoftplusEluOps(NoSoftplusEluOps):
    linear_softplus = True
    linear_elu = True


calls = NoGeluOps                                 # (the counters live there: NoGeluOps.calls)
