"""world_size-2 gloo test of -ts_adapt_wnormtype infinity over batch shards: the ranks agree on the norm with ONE all-reduce (MAX)
per step attempt, and because max is associative the sharded solve takes the full-batch solve's step sequence BITWISE (the
sum of squares of the default norm only to rounding); a NaN on one rank reaches both.  The device ops are the CPU stand-in of
tests/_winf_cases.py."""
import math
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B, TIMES, TOL = 6, [0.0, 0.3, 0.7], 1e-8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _y0():
    g = torch.Generator().manual_seed(5)
    return torch.randn(B, 2, generator=g, dtype=torch.float64) * torch.logspace(-1, 0.2, B, dtype=torch.float64).view(B, 1)


def _solve(y0, group):
    from _winf_cases import Cubic, CpuWinfOps
    from pnode_amd import options, petsc_adjoint
    options.clear()
    for k, v in (("ts_adapt_wnormtype", "infinity"), ("ts_rtol", TOL), ("ts_atol", TOL)):
        options.set_option(k, v)
    try:
        ode = petsc_adjoint.ODEPetsc(backend=CpuWinfOps)
        ode.setupTS(y0, Cubic(), step_size=0.1, method="dopri5")
        if group:
            ode.setProcessGroup(None, average=True, global_error_norm=True)
        with torch.no_grad():
            sol = ode.odeint_adjoint(y0, torch.tensor(TIMES, dtype=torch.float64))
        return ode, {"sol": sol, "log": ode.step_log(), "rej": ode.num_rejections}
    finally:
        options.clear()


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    lo, hi = rank * B // world, (rank + 1) * B // world
    ode, out = _solve(_y0()[lo:hi], True)
    # a NaN on one rank reaches both; a finite norm is the largest of the two
    out["nan"] = ode._global_enorm(float("nan") if rank == 1 else 0.25)
    out["max"] = ode._global_enorm(0.5 if rank == 0 else 0.125)
    out["inf"] = ode._global_enorm(float("inf") if rank == 0 else 2.0)
    torch.save(out, out_path % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_takes_the_full_batch_steps_bitwise_and_nan_reaches_both_ranks(tmp_path):
    world = 2
    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    parts = [torch.load(out % r) for r in range(world)]
    sys.path.insert(0, HERE)
    _, full = _solve(_y0(), False)
    assert full["rej"] > 0 and len(full["log"]) > 5
    for p in parts:
        assert p["log"] == full["log"] and p["rej"] == full["rej"]          # floats compared with ==: bitwise
        assert math.isnan(p["nan"]) and p["max"] == 0.5 and p["inf"] == float("inf")
    assert torch.equal(torch.cat([p["sol"] for p in parts], dim=1), full["sol"])
