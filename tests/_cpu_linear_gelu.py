"""TEST SCAFFOLDING -- the CPU stand-in (tests/_cpu_vecops.py) with the entry points of the fused Linear kernels, GELU and the second
output included: ``pn_linear_fwd`` / ``pn_linear_fwd_pre``, ``pn_linear_bwd`` / ``pn_linear_bwd_act`` and ``pn_linear_dx`` are stood in
for by the torch expressions they replace, and every call is counted by name -- ``fwd_gelu`` is the y-only form, ``fwd_gelu_pre`` the one
that also writes the pre-activation."""
import torch
import torch.nn.functional as F

from _cpu_vecops import CpuVecOps

ACT = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, "gelu": F.gelu, "identity": lambda v: v}


def shapes(dtype, rows, out_f, in_f):
    return dtype == torch.float32 and rows >= 256 and out_f % 64 == 0 and in_f % 64 == 0


class NoGeluOps(CpuVecOps):
    """Every entry point and the ReLU and Sigmoid capabilities, but without `linear_gelu`: what a backend built before PN_ACT_GELU looks
    like to the engine (its linear_act_fwd still takes the name: the forward asks for no capability, as the Sigmoid pairs')."""
    linear_relu = True
    linear_sigmoid = True
    calls = {}

    @classmethod
    def count(cls, what):
        NoGeluOps.calls[what] = NoGeluOps.calls.get(what, 0) + 1

    def linear_fwd_supported(self, rows, out_f, in_f):
        return shapes(self.dtype, rows, out_f, in_f)

    def linear_fwd(self, x, w, b, tanh, y=None, flags=None, act=None):
        assert act != "gelu"                      # (HipVecOps.linear_fwd refuses the name: the GELU pairs go through linear_act_fwd)
        return self.linear_act_fwd(x, w, b, act if act is not None else ("tanh" if tanh else "identity"))

    def linear_act_fwd(self, x, w, b, act, y=None, z=None, flags=None):
        assert self.linear_fwd_supported(x.shape[0], w.shape[0], w.shape[1]) and x.dim() == 2 and x.is_contiguous()
        self.count("fwd_" + act + ("" if z is None else "_pre"))
        lin = F.linear(x, w, b)
        if z is not None:
            assert z.shape == lin.shape and z.is_contiguous()
            z.copy_(lin)
        return ACT[act](lin)

    def linear_bwd_supported(self, rows, out_f, in_f):
        return shapes(self.dtype, rows, out_f, in_f)

    def linear_bwd(self, g, a, w, gz=None, dx=None, flags=None, act="tanh"):
        assert g.dim() == 2 and g.is_contiguous() and a.shape == g.shape
        self.count("bwd_" + act)
        if act == "gelu":
            gz = torch.ops.aten.gelu_backward(g, a, approximate="none")          # (a: the pre-activation)
        elif act == "sigmoid":
            gz = torch.ops.aten.sigmoid_backward(g, a)
        else:
            gz = torch.ops.aten.threshold_backward(g, a, 0) if act == "relu" else torch.ops.aten.tanh_backward(g, a)
        return gz, torch.matmul(gz, w)

    def linear_dx_supported(self, rows, out_f, in_f):
        return shapes(self.dtype, rows, out_f, in_f)

    def linear_dx(self, g, w, dx=None, flags=None):
        self.count("dx")
        return torch.matmul(g, w)


class GeluOps(NoGeluOps):
    linear_gelu = True
