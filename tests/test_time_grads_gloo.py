"""world_size-2 gloo test of dL/dt over batch shards: each rank integrates its own half of the batch with
a non-autonomous func; the per-rank dL/dt is summed and averaged over the ranks with dL/dtheta, and equals the dL/dt of the
full-batch solve -- fp64 (one all-reduce with dL/dtheta), fp32 (dL/dt beside it, in double) and a func with no trainable
parameter (dL/dt alone).  The device ops are the CPU stand-in (tests/_cpu_tgrad_ops.py)."""
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
B, D = 8, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class TimeMLP(nn.Module):
    def __init__(self, dtype, trainable=True):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.lin = nn.Linear(D, D)
        with torch.no_grad():
            self.lin.weight.copy_(0.6 * torch.randn(D, D, generator=g, dtype=torch.float64))
            self.lin.bias.copy_(0.3 * torch.randn(D, generator=g, dtype=torch.float64))
        self.to(dtype)
        for p in self.parameters():
            p.requires_grad_(trainable)

    def forward(self, t, y):
        t = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        return torch.tanh(self.lin(y)) * (1.0 + 0.5 * torch.sin(3.0 * t)) + 0.2 * torch.cos(2.0 * t)


def _solve(case, rank, world):
    from _cpu_tgrad_ops import CpuTgradOps
    from pnode_amd import options, petsc_adjoint
    method, mode, adaptive, dtype, trainable = case
    options.clear()
    options.set_option("pn_output_times", mode)
    if not adaptive:
        options.set_option("ts_adapt_type", "none")
    torch.manual_seed(0)
    y0_full = torch.randn(B, D, dtype=torch.float64).to(dtype)
    t = torch.tensor([0.1, 0.33, 0.5, 0.77, 0.9], dtype=torch.float64).to(dtype)
    w_full = torch.linspace(0.5, 1.5, B * D, dtype=torch.float64).view(B, D).to(dtype)
    lo, hi = (rank * B // world, (rank + 1) * B // world) if world > 1 else (0, B)
    f = TimeMLP(dtype, trainable)
    ode = petsc_adjoint.ODEPetsc(backend=CpuTgradOps)
    ode.setupTS(y0_full[lo:hi], f, step_size=0.05, method=method)
    if world > 1:
        ode.setProcessGroup(None, average=True, global_error_norm=True)
    y = y0_full[lo:hi].clone().requires_grad_(True)
    tt = t.clone().requires_grad_(True)
    pred = ode.odeint_adjoint(y, tt)
    # the mean over the shard: averaged over the ranks, the gradient of the mean over the full batch
    (sum((pred[i] * w_full[lo:hi] * (1 + 0.1 * i)).sum() for i in range(pred.shape[0])) / ((hi - lo) * D)).backward()
    options.clear()
    return {"gt": tt.grad.clone(), "gp": [p.grad.clone() for p in f.parameters() if p.grad is not None], "np": ode.np}


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


@pytest.mark.parametrize("case", [
    ("rk4", "match", False, torch.float64, True),
    ("dopri5", "match", True, torch.float64, True),
    ("dopri5", "interpolate", True, torch.float64, True),
    ("rk4", "match", False, torch.float32, True),
    ("rk4", "match", False, torch.float64, False),
], ids=["rk4-fp64", "dopri5-fp64", "dopri5-interpolate-fp64", "rk4-fp32", "rk4-fp64-no-parameters"])
def test_sharded_t_grad_equals_the_full_batch(tmp_path, case):
    world = 2
    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_worker, args=(world, _free_port(), case, out), nprocs=world, join=True)
    parts = [torch.load(out % r) for r in range(world)]
    sys.path.insert(0, HERE)
    full = _solve(case, 0, 1)
    tol = 1e-5 if case[3] == torch.float32 else 1e-12
    assert torch.equal(parts[0]["gt"], parts[1]["gt"])
    assert parts[0]["gt"].dtype == case[3]
    assert float((parts[0]["gt"] - full["gt"]).abs().max()) <= tol * float(full["gt"].abs().max())
    if case[4]:
        for a, b in zip(parts[0]["gp"], full["gp"]):
            assert float((a - b).abs().max()) <= tol * float(b.abs().max())
    else:
        assert parts[0]["np"] == 0 and not parts[0]["gp"]
