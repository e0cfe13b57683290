"""TEST SCAFFOLDING -- the batches and the solve of tests/test_rows_compact.py and tests/test_gpu_rows_compact.py
(-pn_rows_compact 0|1).

Two kinds of func.  The cubic spiral of tests/test_sample_adapt.py is row-independent to the bit in fp64 (that file asserts it with
torch.equal on sub-batches): with it -pn_rows_compact 1 must reproduce 0 exactly; SpiralElementwise is the same right-hand side
built so that this holds in every dtype and on every device.  The time-dependent spiral of tests/test_sample_time_grads.py sends
<w, df/dt> per row through the scatter; its drift's gradient is a sum over the rows func was given and rounds with their number.
RateMLP is a small MLP with parameters whose rows carry their own rate in the state (dk/dt = 0): the rates are spread
over a factor of 60, so the rows' step counts are, and its Linear layers go through the library's GEMM, whose rounding may depend on
the number of rows: 1 agrees with 0 to round-off."""
import torch
import torch.nn as nn

from problems import SpiralTruth, flat_grads
from pnode_amd import options, petsc_adjoint

TIMES = [0.0, 0.05, 0.12, 0.2]
TOL = {"3bs": 1e-6, "5dp": 1e-8}
RATES = [0.5, 0.7, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 12.0, 18.0, 24.0, 30.0]      # the first B of these


class TimeSpiral(nn.Module):
    """tests/test_sample_time_grads.py's func: the spiral times a factor in t, plus a drift in t (t broadcasts against the rows)."""

    def __init__(self, dtype=torch.float64):
        super().__init__()
        self.inner = SpiralTruth(dtype)
        self.v = nn.Parameter(torch.tensor([0.3, -0.2], dtype=dtype))

    def forward(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype)
        return self.inner(t, y) * (1.0 + 0.5 * torch.sin(5.0 * t)) + self.v * torch.cos(3.0 * t)


class SpiralElementwise(nn.Module):
    """The cubic spiral y' = y**3 A without a matrix product: every entry of a row's result comes from that row's entries through
    elementwise operations alone, so a row's bits cannot depend on the number of rows whatever library serves the call (a GEMM picks
    its kernel, and with it its rounding, by the row count -- in fp32 the CPU's does).  dL/dA still sums over the rows func was given."""

    def __init__(self, dtype=torch.float64):
        super().__init__()
        self.A = nn.Parameter(torch.tensor([[-0.1, 2.0], [-2.0, -0.1]], dtype=dtype))

    def forward(self, t, y):
        c = y ** 3
        a, b = c[..., 0:1], c[..., 1:2]
        return torch.cat([a * self.A[0, 0] + b * self.A[1, 0], a * self.A[0, 1] + b * self.A[1, 1]], dim=-1)


class RateMLP(nn.Module):
    """State rows (x_0 .. x_{w-1}, k): dx/dt = k * (W2 tanh(W1 x + b1) + b2 - x), dk/dt = 0."""

    def __init__(self, width=3, hidden=8, dtype=torch.float64, seed=3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.l1, self.l2 = nn.Linear(width, hidden).to(dtype), nn.Linear(hidden, width).to(dtype)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64).to(dtype) * 0.8)

    def forward(self, t, y):
        x, k = y[..., :-1], y[..., -1:]
        return torch.cat([k * (self.l2(torch.tanh(self.l1(x))) - x), torch.zeros_like(k)], dim=-1)


class Recording(nn.Module):
    """The spiral, noting the shapes it is called with."""

    def __init__(self):
        super().__init__()
        self.inner = SpiralTruth()
        self.shapes = []

    def forward(self, t, y):
        self.shapes.append((tuple(y.shape), tuple(torch.as_tensor(t).shape)))
        return self.inner(t, y)


def spiral_y0(B, dtype=torch.float64):
    """tests/test_sample_adapt.py's batch: radii spread over 0.05 .. 2 (a batch of one: its outermost row)"""
    g = torch.Generator().manual_seed(0)
    r = torch.logspace(-1.3, 0.3, B, dtype=torch.float64) if B > 1 else torch.tensor([2.0], dtype=torch.float64)
    ang = 6.28 * torch.rand(B, generator=g, dtype=torch.float64)
    return torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=1).to(dtype)


def mlp_y0(B, width=3, dtype=torch.float64):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, width, generator=g, dtype=torch.float64)
    return torch.cat([x, torch.tensor(RATES[:B], dtype=torch.float64).view(B, 1)], dim=1).to(dtype)


FUNCS = {"spiral": (SpiralTruth, spiral_y0), "time": (TimeSpiral, spiral_y0), "mlp": (RateMLP, mlp_y0),
         "elementwise": (SpiralElementwise, spiral_y0)}


def solve(backend, compact, func="spiral", B=8, rk="5dp", extra=(), tgrad=False, times=TIMES, step_size=0.01, tol=None, device=None,
          dtype=torch.float64, module=None):
    """One per-sample solve and its backward; `compact` None leaves the option out, else it is passed as given.  loss = sum(pred * w)
    with per-row weights (rows do not mix)."""
    options.clear()
    options.set_option("ts_rk_type", rk)
    tol = TOL[rk] if tol is None else tol
    options.set_option("ts_rtol", tol)
    options.set_option("ts_atol", tol)
    options.set_option("pn_adapt_scope", "sample")
    for k, v in extra:
        options.set_option(k, v)
    if compact is not None:
        options.set_option("pn_rows_compact", compact)
    try:
        make, y0 = FUNCS[func]
        f = make() if module is None else module
        if module is None and dtype != torch.float64:
            f = make(dtype=dtype)
        y = y0(B, dtype=dtype)
        g = torch.Generator().manual_seed(7)
        w = (torch.rand((len(times),) + tuple(y.shape), generator=g, dtype=torch.float64) + 0.5).to(dtype)
        if device is not None:
            f, y, w = f.to(device), y.to(device), w.to(device)
        ode = petsc_adjoint.ODEPetsc(**({} if backend is None else {"backend": backend}))
        y = y.requires_grad_(True)
        ode.setupTS(y, f, step_size=step_size, method="dopri5", enable_adjoint=True)
        t = torch.tensor(times, dtype=torch.float64, device=y.device, requires_grad=tgrad)
        pred = ode.odeint_adjoint(y, t)
        (pred * w).sum().backward()
        return {"ode": ode, "f": f, "sol": pred.detach().clone(), "gu": y.grad.clone(), "gp": flat_grads(f).clone(),
                "gt": t.grad.clone() if tgrad else None,
                "dtrow": ode.sample_time_grads.clone() if tgrad and ode.sample_time_grads is not None else None,
                "logs": [ode.sample_step_log(r) for r in range(B)]}
    finally:
        options.clear()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
