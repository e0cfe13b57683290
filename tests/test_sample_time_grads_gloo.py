"""world_size-2 gloo test of dL/dt of a -pn_adapt_scope sample solve over batch shards: each rank integrates
its own half of the rows; the per-rank dL/dt is summed over the ranks with dL/dtheta (fp64: one all-reduce; fp32: beside it, in
double) and equals the dL/dt of the full-batch solve, while `sample_time_grads` stays the rank's own columns.  The device ops
are the CPU stand-in (tests/_cpu_rows_tgrad_ops.py)."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B = 6
TIMES = [0.0, 0.05, 0.12, 0.2]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class TimeSpiral(nn.Module):
    def __init__(self, dtype):
        super().__init__()
        from problems import SpiralTruth
        self.inner = SpiralTruth(dtype)
        self.v = nn.Parameter(torch.tensor([0.3, -0.2], dtype=dtype))

    def forward(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype)
        return self.inner(t, y) * (1.0 + 0.5 * torch.sin(5.0 * t)) + self.v * torch.cos(3.0 * t)


def _solve(case, rank, world):
    from _cpu_rows_tgrad_ops import CpuRowsTgradOps
    from problems import flat_grads
    from pnode_amd import options, petsc_adjoint
    mode, dtype, tol = case
    options.clear()
    options.set_option("ts_rk_type", "5dp")
    options.set_option("ts_rtol", tol)
    options.set_option("ts_atol", tol)
    options.set_option("pn_adapt_scope", "sample")
    options.set_option("pn_output_times", mode)
    g = torch.Generator().manual_seed(0)
    r = torch.logspace(-1.3, 0.3, B, dtype=torch.float64)
    ang = 6.28 * torch.rand(B, generator=g, dtype=torch.float64)
    y0_full = torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=1).to(dtype)
    w_full = (torch.rand(len(TIMES), B, 2, generator=torch.Generator().manual_seed(7), dtype=torch.float64) + 0.5).to(dtype)
    lo, hi = (rank * B // world, (rank + 1) * B // world) if world > 1 else (0, B)
    f = TimeSpiral(dtype)
    ode = petsc_adjoint.ODEPetsc(backend=CpuRowsTgradOps)
    ode.setupTS(y0_full[lo:hi], f, step_size=0.2, method="dopri5")
    if world > 1:
        ode.setProcessGroup(None, average=False, global_error_norm=True)
    y = y0_full[lo:hi].clone().requires_grad_(True)
    t = torch.tensor(TIMES, dtype=torch.float64, requires_grad=True)
    pred = ode.odeint_adjoint(y, t)
    (pred * w_full[:, lo:hi]).sum().backward()
    options.clear()
    return {"gt": t.grad.clone(), "gp": flat_grads(f).clone(), "dtrow": ode.sample_time_grads.clone(), "rows": (lo, hi)}


def _worker(rank, world, port, case, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.save(_solve(case, rank, world), out_path % rank)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", [("match", torch.float64, 1e-8), ("interpolate", torch.float64, 1e-8), ("match", torch.float32, 1e-4)],
                         ids=["match-fp64", "interpolate-fp64", "match-fp32"])
def test_sharded_sample_t_grad_equals_the_full_batch(tmp_path, case):
    world = 2
    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_worker, args=(world, _free_port(), case, out), nprocs=world, join=True)
    parts = [torch.load(out % r) for r in range(world)]
    sys.path.insert(0, HERE)
    full = _solve(case, 0, 1)
    assert torch.equal(parts[0]["gt"], parts[1]["gt"]) and parts[0]["gt"].dtype == torch.float64
    # the rank's columns are the full solve's, bit for bit (a row does not depend on its batch), and stay local
    for p in parts:
        lo, hi = p["rows"]
        assert p["dtrow"].shape == (len(TIMES), hi - lo) and torch.equal(p["dtrow"], full["dtrow"][:, lo:hi])
    # the same B numbers per entry added in another order: (B - 1) 2^-53 sum_r |dtrow[i, r]| (tests/test_sample_time_grads.py)
    bound = (B - 1) * 2.0 ** -53 * full["dtrow"].abs().sum(1)
    assert bool(((parts[0]["gt"] - full["gt"]).abs() <= bound).all()), (parts[0]["gt"], full["gt"])
    tol = 1e-5 if case[1] == torch.float32 else 1e-12
    assert float((parts[0]["gp"] - full["gp"]).abs().max()) <= tol * float(full["gp"].abs().max())
