"""Per-component tolerances without a GPU (ODEPetsc.setTolerances) on the CPU stand-in of
tests/_cpu_vtol_ops.py: the exact identities (constant vectors are the scalar path; power-of-two rescaling), that the vectors
matter on a problem of ROBER's scales, and the surface -- every refusal by message, persistence across setupTS, the way back to the
scalar launches, the status strings, theta / ARKIMEX, and a two-rank gloo solve.  The kernels: tests/test_gpu_vector_tolerances.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import _vtol_cases as vc
from _cpu_vtol_ops import CpuVtolOps
from _winf_cases import CpuWinfOps
from pnode_amd import options, petsc_adjoint
from pnode_amd._lib import PnError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.float64]
NP = {torch.float32: np.float32, torch.float64: np.float64}
TOL = {"5dp": 1e-6, "3bs": 1e-4}


def _f64(x):
    return torch.tensor(x, dtype=torch.float64)


def _c(shape, value):
    return torch.full(shape, value, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------- 1. constant vectors
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", ["2", "infinity"])
def test_kernel_level_constant_vectors_are_the_scalar_entry_points(dtype, norm):
    T = NP[dtype]
    atol, rtol = 3e-4, 7e-4
    for n, p, nk in ((7, 1, 1), (12, 3, 7), (1000, 1000, 7)):
        u, K, cb, ce = vc.operands(T, n, nk, seed=n)
        ops = CpuVtolOps(CPU, dtype, n)
        tu, tK = torch.from_numpy(u), [torch.from_numpy(k) for k in K]
        a, b = torch.empty(n, dtype=dtype), torch.empty(n, dtype=dtype)
        va, vr = torch.full((p,), atol, dtype=torch.float64), torch.full((p,), rtol, dtype=torch.float64)
        if norm == "2":
            ops.combine_wrms(a, tu, tK, cb, ce, atol, rtol)
            want = ops.read_enorm()
            ops.combine_wrms_v(b, tu, tK, cb, ce, va, vr)
            got = ops.read_enorm()
        else:
            ops.combine_winf(a, tu, tK, cb, ce, atol, rtol)
            want = ops.read_enorm_inf()
            ops.combine_winf_v(b, tu, tK, cb, ce, va, vr)
            got = ops.read_enorm_inf()
        assert got == want and want > 0 and torch.equal(a, b)
    B, d = 5, 7
    u, K, cb, ce = vc.operands(T, B * d, 3, seed=5)
    ops = CpuVtolOps(CPU, dtype, B * d)
    h = _f64([0.5, 1.0, 2.0, 1.0, 0.5])
    e1, e2 = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    a, b = torch.empty(B * d, dtype=dtype), torch.empty(B * d, dtype=dtype)
    args = (B, d, a, torch.from_numpy(u), [torch.from_numpy(k) for k in K], cb, ce, h)
    args2 = (B, d, b) + args[3:]
    va, vr = torch.full((d,), atol, dtype=torch.float64), torch.full((d,), rtol, dtype=torch.float64)
    if norm == "2":
        ops.rows_combine_wrms(*args, atol, rtol, e1)
        ops.rows_combine_wrms_v(*args2, va, vr, e2)
    else:
        ops.rows_combine_winf(*args, atol, rtol, e1)
        ops.rows_combine_winf_v(*args2, va, vr, e2)
    assert torch.equal(e1, e2) and bool((e1 > 0).all()) and torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", ["2", "infinity"])
@pytest.mark.parametrize("scope", ["batch", "sample"])
@pytest.mark.parametrize("rk", ["3bs", "5dp"])
def test_solve_level_constant_vectors_are_the_scalar_solve(rk, scope, norm, dtype):
    y0, tol = vc.y0_mix(dtype), TOL[rk]
    scalar = vc.solve(y0, vc.Mix(dtype), rk, scope, norm, tol=(tol, tol), backend=CpuVtolOps, step_size=0.5)
    assert scalar["status"] == "scalar (atol %g, rtol %g)" % (tol, tol)
    # rtol with the shape of one sample; atol with the shape of the whole state (batch scope) or of one sample (sample scope)
    vtol = (_c((3,), tol), _c((3,) if scope == "sample" else (5, 3), tol))
    vec = vc.solve(y0, vc.Mix(dtype), rk, scope, norm, tol=(1e-2, 1e-2), vtol=vtol, backend=CpuVtolOps, step_size=0.5)
    assert vec["status"].startswith("vector (period %d of n 15; atol %g, rtol %g" % (3 if scope == "sample" else 15, tol, tol))
    vc.same_solve(scalar, vec)
    calls = vec["ode"]._ops.calls
    name = ("rows_" if scope == "sample" else "") + ("combine_winf" if norm == "infinity" else "combine_wrms")
    assert calls.get(name + "_v", 0) > 0 and not calls.get(name, 0)
    assert (sum(scalar["counts"][1]) if scope == "sample" else scalar["counts"][1]) > 0          # rejections are part of what is compared


def test_a_solve_that_never_calls_setTolerances_launches_what_it_launched():
    y0 = vc.y0_mix(torch.float64)
    out = vc.solve(y0, vc.Mix(torch.float64), backend=CpuVtolOps)
    calls = out["ode"]._ops.calls
    assert calls["combine_wrms"] > 0 and not any(k.endswith("_v") for k in calls)
    assert out["ode"]._native and out["ode"]._vtol is None


# ---------------------------------------------------------------------------------------------------- 2. power-of-two rescaling
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", ["2", "infinity"])
@pytest.mark.parametrize("scope", ["batch", "sample"])
def test_power_of_two_rescaling_solve(scope, norm, dtype):
    """u under atol_e = s_e a against v = u / s under the scalar a, g(t, v) = f(t, s v) / s: the same steps, the same rejections,
    u == s v bit for bit."""
    a, rtol = 1e-6, 1e-6
    s = torch.tensor(vc.SCALES, dtype=dtype)
    y0 = vc.y0_mix(dtype)
    big = vc.solve(y0, vc.Mix(dtype), "5dp", scope, norm, tol=(rtol, 1e-2), vtol=(None, a * s.double()), backend=CpuVtolOps, grad=False, step_size=0.5)
    small = vc.solve(y0 / s, vc.Mix(dtype, vc.SCALES), "5dp", scope, norm, tol=(rtol, a), backend=CpuVtolOps, grad=False, step_size=0.5)
    assert big["log"] == small["log"] and big["counts"] == small["counts"]
    assert torch.equal(big["sol"], small["sol"] * s)
    assert (sum(big["counts"][1]) if scope == "sample" else big["counts"][1]) > 0
    plain = vc.solve(y0, vc.Mix(dtype), "5dp", scope, norm, tol=(rtol, a), backend=CpuVtolOps, grad=False, step_size=0.5)
    assert plain["log"] != big["log"]                                                # the vector is not the scalar a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", ["2", "infinity"])
def test_power_of_two_rescaling_kernel_level(dtype, norm):
    T, B, d, nk = NP[dtype], 6, 3, 7
    n = B * d
    u, K, cb, ce = vc.operands(T, n, nk, seed=3)
    s = np.tile(np.array(vc.SCALES, dtype=T), B)
    a, rtol = 1e-3, 1e-3
    ops = CpuVtolOps(CPU, dtype, n)
    va, vr = _f64(a * np.array(vc.SCALES)), torch.full((d,), rtol, dtype=torch.float64)
    x, y = torch.empty(n, dtype=dtype), torch.empty(n, dtype=dtype)
    tn = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    if norm == "2":
        ops.combine_wrms_v(x, tn(u), [tn(k) for k in K], cb, ce, va, vr)
        got = ops.read_enorm()
        ops.combine_wrms(y, tn(u / s), [tn(k / s) for k in K], cb, ce, a, rtol)
        want = ops.read_enorm()
    else:
        ops.combine_winf_v(x, tn(u), [tn(k) for k in K], cb, ce, va, vr)
        got = ops.read_enorm_inf()
        ops.combine_winf(y, tn(u / s), [tn(k / s) for k in K], cb, ce, a, rtol)
        want = ops.read_enorm_inf()
    assert got == want and want > 0 and torch.equal(x, y * tn(s))


# ---------------------------------------------------------------------------------------------------- 3. it matters
def test_a_small_atol_for_the_small_species_costs_steps_between_the_two_scalars():
    B = 8
    y0 = torch.zeros(B, 3, dtype=torch.float64)
    y0[:, 0] = torch.linspace(0.9, 1.1, B, dtype=torch.float64)
    steps = []
    for atol in (1e-8, _f64([1e-8, 1e-12, 1e-8]), 1e-12):
        out = vc.solve(y0, vc.Rober(), "5dp", tol=(1e-6, 1e-8), vtol=(1e-6, atol), backend=CpuVtolOps, times=(0.0, 0.01), grad=False,
                       step_size=1e-5)
        steps.append(out["counts"][0])
    print("accepted steps: scalar 1e-8 %d, vector %d, scalar 1e-12 %d" % tuple(steps))
    assert steps[0] < steps[1] < steps[2]


# ---------------------------------------------------------------------------------------------------- 4. the surface
def _ode(y0=None, scope="batch", backend=CpuVtolOps, opts=()):
    options.clear()
    options.set_option("pn_adapt_scope", scope)
    for k, v in opts:
        options.set_option(k, v)
    y0 = vc.y0_mix(torch.float64) if y0 is None else y0
    ode = petsc_adjoint.ODEPetsc(backend=backend)
    ode.setupTS(y0, vc.Mix(y0.dtype), step_size=0.05, method="dopri5")
    return ode, y0


@pytest.fixture
def clean_options():
    yield
    options.clear()


def test_every_refusal_names_what_is_wrong(clean_options):
    with pytest.raises(PnError, match="call setupTS first"):
        petsc_adjoint.ODEPetsc(backend=CpuVtolOps).setTolerances(rtol=1e-3)
    ode, y0 = _ode()
    ok = torch.full((3,), 1e-6, dtype=torch.float64)
    bad = [
        (dict(atol=torch.ones(4, dtype=torch.float64)), r"atol has shape \(4,\); the state has shape \(5, 3\)"),
        (dict(rtol=torch.ones(3, 5, dtype=torch.float64)), r"rtol has shape \(3, 5\)"),
        (dict(atol=ok.clone().requires_grad_(True)), "atol requires grad"),
        (dict(atol=torch.tensor([1e-6, -1e-6, 1e-6])), "every entry of atol must be finite and not negative"),
        (dict(rtol=torch.tensor([1e-6, float("nan"), 1e-6])), "every entry of rtol must be finite and not negative"),
        (dict(atol=torch.tensor([1e-6, float("inf"), 1e-6])), "every entry of atol must be finite"),
        (dict(atol=torch.tensor([1e-6, 0.0, 1e-6]), rtol=0.0), r"atol \+ rtol must be positive for every entry \(entry 1 of the period of 3"),
        (dict(atol=-1.0), "atol must be finite and not negative"),
        (dict(rtol=float("nan")), "rtol must be finite and not negative"),
        (dict(atol=0.0, rtol=0.0), r"atol \+ rtol must be positive"),
        (dict(atol="tight"), "atol must be None, a float or a tensor"),
        (dict(atol=torch.ones(3, dtype=torch.float64, device="meta")), "atol is on meta, the state on cpu"),
    ]
    for kw, text in bad:
        with pytest.raises(PnError, match=text):
            ode.setTolerances(**kw)
        assert ode.tolerances == "scalar (atol 0.0001, rtol 0.0001)", kw                 # a refused call changes nothing
    ode2, _ = _ode(backend=CpuWinfOps)
    with pytest.raises(PnError, match="the backend CpuWinfOps has no per-component entry points.*rows_combine_winf_v"):
        ode2.setTolerances(atol=ok)
    ode3, _ = _ode(scope="sample")
    with pytest.raises(PnError, match=r"under -pn_adapt_scope sample: atol has the shape of the whole state \(5, 3\).*one sample \(3,\)"):
        ode3.setTolerances(atol=_c((5, 3), 1e-6))
    ode3.setTolerances(atol=ok)
    assert ode3.tolerances == "vector (period 3 of n 15; atol 1e-06, rtol 0.0001)"


def test_status_strings_scalars_periods_and_the_way_back(clean_options):
    ode, y0 = _ode()
    assert ode.tolerances == "scalar (atol 0.0001, rtol 0.0001)"
    ode.setTolerances(rtol=1e-6, atol=torch.tensor(1e-6))                                # a float and a 0-d tensor: the scalar path
    assert ode.tolerances == "scalar (atol 1e-06, rtol 1e-06)" and ode._vtol is None
    ode.setTolerances(rtol=1e-4, atol=_f64([1e-14, 1e-6, 1e-10]))
    assert ode.tolerances == "vector (period 3 of n 15; atol 1e-14 … 1e-06, rtol 0.0001; forward attempts: Python stage loop)"
    assert ode._vtol[0].dtype == torch.float64 and ode._vtol[1].tolist() == [1e-4] * 3
    # a whole-state rtol beside the one-sample atol: one common period, the sample repeated over the rows
    ode.setTolerances(rtol=_c((5, 3), 1e-5))
    assert ode._vtol[0].numel() == ode._vtol[1].numel() == 15 and ode._vtol[0].tolist() == [1e-14, 1e-6, 1e-10] * 5
    assert ode.tolerances.startswith("vector (period 15 of n 15; atol 1e-14 … 1e-06, rtol 1e-05")
    ode.setTolerances(atol=1e-7)                                                         # rtol is still a tensor
    assert ode.tolerances.startswith("vector (period 15 of n 15; atol 1e-07, rtol 1e-05")
    ode.setTolerances(rtol=1e-5, atol=1e-7)                                              # two floats: back to the scalar launches
    assert ode.tolerances == "scalar (atol 1e-07, rtol 1e-05)" and ode._vtol is None
    pred = ode.odeint_adjoint(y0.clone().requires_grad_(True), _f64(vc.TIMES))
    calls = ode._ops.calls
    assert calls["combine_wrms"] > 0 and not any(k.endswith("_v") for k in calls) and pred.shape == (3, 5, 3)
    # ... with the numbers of the options: a solver that was given 1e-5 / 1e-7 from the start
    ref = vc.solve(y0, vc.Mix(torch.float64), tol=(1e-5, 1e-7), backend=CpuVtolOps, grad=False)
    assert torch.equal(pred.detach(), ref["sol"]) and ode.step_log() == ref["log"]


def test_the_setting_holds_across_setupTS_and_a_state_that_no_longer_fits_is_refused(clean_options):
    ode, y0 = _ode()
    ode.setTolerances(atol=_f64([1e-9, 1e-6, 1e-7]))
    want = ode.tolerances
    f2 = vc.Mix(torch.float64)
    ode.setupTS(y0, f2, step_size=0.05, method="dopri5")                                 # another func, the same state
    assert ode.tolerances == want
    options.set_option("ts_rtol", 1e-5)                                                  # the options change: re-parsed, the vector stays
    ode.setupTS(y0, f2, step_size=0.05, method="dopri5")
    assert ode.tolerances == want.replace("rtol 0.0001", "rtol 1e-05")
    y8 = torch.cat([y0, y0[:3]])                                                         # more rows: one sample still fits
    ode.setupTS(y8, f2, step_size=0.05, method="dopri5")
    assert ode.tolerances.startswith("vector (period 3 of n 24;")
    with pytest.raises(PnError, match=r"atol has shape \(3,\); the state has shape \(8, 4\)"):
        ode.setupTS(torch.ones(8, 4, dtype=torch.float64), f2, step_size=0.05, method="dopri5")
    with pytest.raises(PnError, match=r"atol has shape \(3,\)"):                         # and keeps being refused
        ode.setupTS(torch.ones(8, 4, dtype=torch.float64), f2, step_size=0.05, method="dopri5")
    ode.setupTS(y8, f2, step_size=0.05, method="dopri5")
    assert ode.tolerances.startswith("vector (period 3 of n 24;")


def test_ts_view_prints_the_status(capsys):
    out = vc.solve(vc.y0_mix(torch.float64), vc.Mix(torch.float64), vtol=(None, _f64([1e-9, 1e-6, 1e-7])), backend=CpuVtolOps, grad=False,
                   extra=(("ts_view", ""),))
    assert "  tolerances: " + out["status"] in capsys.readouterr().out and out["status"].startswith("vector (period 3 of n 15")


def test_fixed_step_solves_ignore_the_vectors():
    y0 = vc.y0_mix(torch.float64)
    kw = dict(rk="4", backend=CpuVtolOps, extra=(("ts_adapt_type", "none"),), method="rk4")
    a = vc.solve(y0, vc.Mix(torch.float64), **kw)
    b = vc.solve(y0, vc.Mix(torch.float64), vtol=(None, _f64([1e-9, 1e-6, 1e-7])), **kw)
    vc.same_solve(a, b)
    assert not any(k.startswith("combine_w") for k, v in b["ode"]._ops.calls.items() if v)


class _Lin(nn.Module):
    def __init__(self, scale):
        super().__init__()
        self.A = nn.Parameter(scale * torch.tensor([[-0.5, 3.0, 0.0], [-3.0, -0.5, 0.2], [0.0, -0.2, -0.1]], dtype=torch.float64))

    def forward(self, t, y):
        return y @ self.A


@pytest.mark.parametrize("norm", ["2", "infinity"])
@pytest.mark.parametrize("kind", ["cn", "arkimex"])
def test_theta_and_arkimex_take_the_vectors_through_the_one_place(kind, norm):
    y0 = vc.y0_mix(torch.float64)
    if kind == "cn":
        kw = dict(rk=None, extra=(("ts_adapt_type", "basic"),), method="cn", setup_kw={"implicit_form": True}, tol=(1e-5, 1e-5))
        f = lambda: _Lin(1.0)
    else:
        kw = dict(rk=None, extra=(("ts_arkimex_type", "3"),), method="imex", tol=(1e-6, 1e-6))
        f = lambda: _Lin(1.0)
    import warnings
    outs = []
    for vt in (None, (_c((3,), kw["tol"][0]), _c((5, 3), kw["tol"][1]))):
        k2 = dict(kw)
        if kind == "arkimex":
            k2["setup_kw"] = {"imex_form": True, "func2": _Lin(0.3), "linear_solver": "torch"}
        if vt is not None:
            k2["tol"] = (1e-2, 1e-2)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs.append(vc.solve(y0, f(), norm=norm, vtol=vt, backend=CpuVtolOps, times=(0.0, 0.5), grad=False, **k2))
    a, b = outs
    assert a["log"] == b["log"] and a["counts"] == b["counts"] and len(a["log"]) > 3 and torch.equal(a["sol"], b["sol"])
    name = "combine_winf" if norm == "infinity" else "combine_wrms"
    assert b["ode"]._ops.calls.get(name + "_v", 0) > 0 and not b["ode"]._ops.calls.get(name, 0)
    assert "Python stage loop" not in b["status"]


# ---------------------------------------------------------------------------------------------------- 5. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_solve(rank, world):
    from problems import SpiralTruth, flat_grads
    options.clear()
    torch.manual_seed(0)
    B = 12
    y0_full = torch.randn(B, 2, dtype=torch.float64)
    t = torch.tensor([0.0, 0.3, 1.0], dtype=torch.float64)
    target_full = torch.randn(3, B, 2, dtype=torch.float64)
    lo, hi = (rank * B // world, (rank + 1) * B // world) if world > 1 else (0, B)
    f = SpiralTruth()
    ode = petsc_adjoint.ODEPetsc(backend=CpuVtolOps)
    ode.setupTS(y0_full[lo:hi], f, step_size=0.1, method="dopri5")
    ode.setTolerances(rtol=1e-5, atol=torch.tensor([1e-7, 1e-4], dtype=torch.float64))     # one sample: the rank's own shard uses it
    if world > 1:
        ode.setProcessGroup(None, average=True, global_error_norm=True)
    y = y0_full[lo:hi].clone().requires_grad_(True)
    pred = ode.odeint_adjoint(y, t)
    torch.mean(torch.abs(pred - target_full[:, lo:hi])).backward()
    return {"pred": pred.detach(), "gy": y.grad, "gtheta": flat_grads(f), "h": [ode._step_info(k)[1] for k in range(ode._nsteps)],
            "rej": ode.num_rejections, "calls": dict(ode._ops.calls)}


def _gloo_worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.save(_gloo_solve(rank, world), out_path % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_with_a_one_sample_vector_equals_the_full_batch_solve(tmp_path):
    """The bars of tests/test_distributed_gloo.py's scalar test, against the full-batch solve under the same vector."""
    from problems import rel_err
    world = 2
    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_gloo_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    parts = [torch.load(out % r) for r in range(world)]
    full = _gloo_solve(0, 1)
    options.clear()
    for p in parts:
        assert len(p["h"]) == len(full["h"]) and p["rej"] == full["rej"] and p["calls"]["combine_wrms_v"] > 0
        assert torch.allclose(_f64(p["h"]), _f64(full["h"]), rtol=1e-10)
    assert full["rej"] > 0
    assert rel_err(torch.cat([p["pred"] for p in parts], dim=1), full["pred"]) < 1e-11
    assert torch.equal(parts[0]["gtheta"], parts[1]["gtheta"]) and rel_err(parts[0]["gtheta"], full["gtheta"]) < 1e-10
    assert rel_err(torch.cat([p["gy"] for p in parts], dim=0) / world, full["gy"]) < 1e-10
