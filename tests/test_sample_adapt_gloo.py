"""world_size-2 gloo test of -pn_adapt_scope sample over batch shards: every rank integrates its own half
of the batch; a row's steps do not depend on the rows beside it, so the sharded states are bitwise those of the unsharded solve
with NO exchange during the sweeps, and dL/dtheta is the one all-reduce of mu.  The device ops are the CPU stand-in
(tests/_cpu_rows_ops.py)."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

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


def _solve(rank, world):
    from _cpu_rows_ops import CpuRowsOps
    from problems import SpiralTruth, flat_grads
    from pnode_amd import options, petsc_adjoint
    options.clear()
    options.set_option("ts_rtol", 1e-8)
    options.set_option("ts_atol", 1e-8)
    options.set_option("pn_adapt_scope", "sample")
    g = torch.Generator().manual_seed(0)
    r = torch.logspace(-1.3, 0.3, B, dtype=torch.float64)
    ang = 6.28 * torch.rand(B, generator=g, dtype=torch.float64)
    y0_full = torch.stack([r * torch.cos(ang), r * torch.sin(ang)], dim=1)
    w_full = torch.rand(len(TIMES), B, 2, generator=g, dtype=torch.float64) + 0.5
    lo, hi = (rank * B // world, (rank + 1) * B // world) if world > 1 else (0, B)
    f = SpiralTruth()
    ode = petsc_adjoint.ODEPetsc(backend=CpuRowsOps)
    ode.setupTS(y0_full[lo:hi], f, step_size=0.01, method="dopri5")
    calls = []
    if world > 1:
        ode.setProcessGroup(None, average=False, global_error_norm=True)
        real = dist.all_reduce
        dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    y = y0_full[lo:hi].clone().requires_grad_(True)
    pred = ode.odeint_adjoint(y, torch.tensor(TIMES, dtype=torch.float64))
    n_forward = len(calls)
    (pred * w_full[:, lo:hi]).sum().backward()
    options.clear()
    return {"sol": pred.detach().clone(), "gu": y.grad.clone(), "gp": flat_grads(f).clone(), "steps": ode.sample_steps.clone(),
            "reduces": (n_forward, len(calls))}


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.save(_solve(rank, world), out_path % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_sample_solve_is_the_unsharded_one(tmp_path):
    world = 2
    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    parts = [torch.load(out % r) for r in range(world)]
    sys.path.insert(0, HERE)
    full = _solve(0, 1)
    assert torch.equal(torch.cat([p["sol"] for p in parts], dim=1), full["sol"])
    gu = torch.cat([p["gu"] for p in parts], dim=0)        # (bitwise across batches within one process: test_sample_adapt.py)
    assert float((gu - full["gu"]).abs().max()) <= 1e-13 * float(full["gu"].abs().max())
    assert torch.equal(torch.cat([p["steps"] for p in parts]), full["steps"])
    for p in parts:
        assert p["reduces"] == (0, 1)                     # no all-reduce per step attempt; mu once per backward
        assert float((p["gp"] - full["gp"]).abs().max()) <= 1e-13 * float(full["gp"].abs().max())
    assert torch.equal(parts[0]["gp"], parts[1]["gp"])
