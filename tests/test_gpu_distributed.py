"""-m gpu: the batch-sharded path with the real HIP backend.  Two ranks share the single GPU of the
test box and talk over gloo (device tensors); on a multi-GPU node the identical code runs one rank
per GPU over RCCL.  Checked against a single-process full-batch solve on the same GPU."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup(method, opts):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from pnode_amd import options
    from problems import SpiralFunc, SpiralTruth
    options.clear()
    for k, v in opts.items():
        options.set_option(k, v)
    torch.manual_seed(0)
    B = 12
    y0 = torch.randn(B, 2, dtype=torch.float64)
    t = torch.tensor([0.0, 0.3, 1.0], dtype=torch.float64)
    target = torch.randn(3, B, 2, dtype=torch.float64)
    f = SpiralFunc() if method == "rk4" else SpiralTruth()
    return y0, t, target, f


def _solve(y0, t, target, f, method, step_size, group_world):
    from pnode_amd import petsc_adjoint
    from problems import flat_grads
    dev = torch.device("cuda:0")
    f = f.to(dev)
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0.to(dev), f, step_size=step_size, method=method)
    if group_world > 1:
        ode.setProcessGroup(None, average=True, global_error_norm=True)
    y = y0.to(dev).requires_grad_(True)
    pred = ode.odeint_adjoint(y, t.to(dev))
    torch.mean(torch.abs(pred - target.to(dev))).backward()
    return {"pred": pred.detach().cpu(), "gy": y.grad.cpu(), "gtheta": flat_grads(f).cpu(),
            "h": [h for _, h in ode.step_log()], "rej": ode.num_rejections}


def _worker(rank, world, port, method, opts, step_size, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    y0, t, target, f = _setup(method, opts)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = rank * y0.shape[0] // world, (rank + 1) * y0.shape[0] // world
    res = _solve(y0[lo:hi], t, target[:, lo:hi], f, method, step_size, world)
    torch.save(res, out_path % rank)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("method,opts,step_size", [
    ("rk4", {"ts_adapt_type": "none"}, 0.05),
    ("dopri5", {}, 0.1),
])
def test_two_ranks_on_the_hip_backend_equal_the_full_batch_solve(tmp_path, method, opts, step_size):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    world = 2
    out = str(tmp_path / "rank%d.pt")
    mp.spawn(_worker, args=(world, _free_port(), method, opts, step_size, out), nprocs=world, join=True)
    parts = [torch.load(out % r) for r in range(world)]
    y0, t, target, f = _setup(method, opts)
    full = _solve(y0, t, target, f, method, step_size, 1)
    from problems import rel_err
    for p in parts:
        assert len(p["h"]) == len(full["h"]) and p["rej"] == full["rej"]
        assert torch.allclose(torch.tensor(p["h"], dtype=torch.float64), torch.tensor(full["h"], dtype=torch.float64), rtol=1e-10)
    if method != "rk4":
        assert full["rej"] > 0
    assert rel_err(torch.cat([p["pred"] for p in parts], dim=1), full["pred"]) < 1e-11
    assert torch.equal(parts[0]["gtheta"], parts[1]["gtheta"])
    assert rel_err(parts[0]["gtheta"], full["gtheta"]) < 1e-10
    assert rel_err(torch.cat([p["gy"] for p in parts], dim=0) / world, full["gy"]) < 1e-10


@pytest.mark.parametrize("strong", [False, True])
def test_bench_contract_with_two_ranks(strong):
    """bench.py launched exactly as the driver launches it for N > 1 (torch.distributed.run, one rank
    per process), with the gloo test hook so that two ranks can share this box's single GPU: one JSON
    line from rank 0 with the whole-job rate, the roofline object and the collective's time."""
    import json
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    env = dict(os.environ, PN_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "256", "--dim", "64", "--nt", "6",
           "--full", "--no-cpu-baseline", "--no-variants"] + (["--strong"] if strong else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "time-steps/s"
    assert d["scaling"] == ("strong" if strong else "weak") and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["config"]["batch_per_gpu"] == (128 if strong else 256) and d["config"]["launch_mode"] == "graph(auto)"
    assert d["config"]["allreduce_us"] > 0 and d["cpu_baseline"] is None
    assert d["value"] == pytest.approx(2 * 6 * 2 / (d["ms_per_step"] * 2 / 1e3), rel=1e-6)
    assert 0 < d["roofline"]["frac"] < 1 and d["roofline"]["bound"] == "hbm"


def test_rccl_world_size_one_full_flow():
    """The real backend of the multi-GPU path -- "nccl" (RCCL) -- on the one GPU of this box: communicator
    creation, setProcessGroup, hipGraph capture and replay with the communicator alive, ncclAllReduce of the
    parameter gradient after every backward, the scalar all-reduce of the adaptive error norm.  With one rank
    the reductions are identities, so the results must equal the solves without a process group bit for bit."""
    import json
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    r = subprocess.run([sys.executable, os.path.join(HERE, "nccl_world1_worker.py"), str(_free_port())],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["backend"] == "nccl" and d["probe"] == 1024.0 and d["rccl_loaded"] and d["pnode_amd_loaded"]
    assert d["rk4_graph_graphs"] is True and d["rk4_graph_world"] == 1
    # rk4: a one-rank sum is the identity.  dopri5: sqrt(sum(n e^2)/sum(n)) may differ from e in the last bit,
    # which moves the step sizes by round-off
    assert d["rk4_graph"] == 0.0 and d["dopri5_global_norm"] < 1e-5
    # cn: a one-rank sum of the Krylov products is the identity; the deferred decisions are the fused ones
    assert d["cn_krylov"] < 1e-6 and d["cn_krylov_its"][1] > 10 and d["cn_krylov_its"][3] > 0


def test_bench_gpus_flag_without_a_launcher_fails_loudly_on_a_one_gpu_box():
    """`python bench.py --gpus 2` must never report a one-GPU run as a two-GPU point.  Without
    WORLD_SIZE the bench starts the ranks itself; with fewer GPUs than ranks it exits non-zero and says why."""
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box with one GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PN_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0
    assert "needs 2 GPUs" in r.stderr and not any(l.startswith("{") for l in r.stdout.splitlines())


def test_bench_self_launch_with_two_ranks():
    """`python bench.py --gpus 2` (no launcher): the parent starts two fresh ranks under torch.distributed.run and
    passes rank 0's JSON line through (gloo test hook: both ranks share this box's GPU)."""
    import json
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PN_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--batch", "256", "--dim", "64", "--nt", "6", "--no-cpu-baseline", "--no-variants"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    assert json.loads(lines[0])["n_gpus"] == 2


def test_bench_config_c4_line():
    """bench.py --config c4: BASELINE config 4's shard (the config that names 8 GPUs) through the same contract."""
    import json
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PN_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c4", "--steps", "2", "--warmup", "1",
                        "--batch", "16", "--full", "--no-cpu-baseline", "--no-variants"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["config"]["workload"].startswith("C4 shard") and d["config"]["time_steps"] == 4
    assert d["config"]["state_elements_per_gpu"] == 16 * 64 * 32 * 32
    assert 0 < d["roofline"]["frac"] < 1.5 and 0 < d["roofline"]["vector_only"]["frac"] < 1.5
    # the profiler child ran and its per-kernel table holds the solver kernels of the timed (graph-replayed) region
    rp = d["roofline"]["rocprofv3"]
    assert rp is not None and d["roofline"]["frac"] == rp["frac"] and d["roofline"]["hip_events"]["frac"] > 0
    assert any(k.startswith("pn_lincomb_kernel") for k in rp["per_kernel"])


def _run_bench(argv, env=None, launcher=None):
    import json
    import subprocess
    cmd = ([sys.executable] + (launcher or []) + [os.path.join(ROOT, "bench.py")] + argv)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, **(env or {})), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("config,extra", [("c3b", ["--batch", "128", "--dim", "32"]), ("c5", ["--batch", "8", "--nt", "3"])])
def test_bench_two_ranks_on_the_configs_that_add_a_collective_or_name_eight_gpus(config, extra):
    """`--config c3b` (config 3 as written: adaptive, one scalar all-reduce per step attempt when
    sharded) and `--config c5` (the Burgers IMEX shard, the config that names 8 GPUs) under the driver's N > 1 launch
    line, two ranks sharing this box's GPU over gloo."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    launcher = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(_free_port())]
    d = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--config", config, "--full", "--no-cpu-baseline", "--no-variants"] + extra,
                   env={"PN_BENCH_BACKEND": "gloo"}, launcher=launcher)
    assert d["n_gpus"] == 2 and d["unit"] == "time-steps/s" and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["config"]["allreduce_us"] > 0 and d["cpu_baseline"] is None
    assert d["value"] == pytest.approx(2 * d["config"]["time_steps"] * 2 / (d["ms_per_step"] * 2 / 1e3), rel=1e-6)
    assert 0 < d["roofline"]["frac"] < 1 and d["roofline"]["bound"] == "hbm" and d["roofline"]["traffic"] is None
    if config == "c3b":
        assert d["dtype"] == "f32" and d["config"]["enorm_allreduce_us"] > 0 and d["config"]["launch_mode"].startswith("eager")
        assert d["config"]["time_steps"] >= 2 and "dopri5" in d["config"]["workload"]
    else:
        assert d["dtype"] == "f64" and d["config"]["time_steps"] == 3 and d["config"]["enorm_allreduce_us"] is None
        assert "ARKIMEX" in d["config"]["workload"]


@pytest.mark.parametrize("config,extra", [("c2", ["--batch", "256", "--nt", "6"]), ("c3b", ["--batch", "128", "--dim", "32"]),
                                          ("c5", ["--batch", "8", "--nt", "3"]), ("c3a", ["--batch", "256", "--dim", "64", "--nt", "6"])])
def test_bench_single_rank_configs_and_the_measured_parts_of_the_line(config, extra):
    """One rank, every config the bench knows: the JSON contract, `roofline.traffic` MEASURED in the run (two rocprofv3 --pmc
    children) or null -- never a committed constant --, the profiler child's kernel durations, and for the headline config
    the same solve in the reference's CI precision (`variants.f64`) with its own roofline."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    d = _run_bench(["--steps", "3", "--warmup", "1", "--config", config, "--full", "--no-cpu-baseline"] + extra +
                   ([] if config == "c3a" else ["--no-ceiling"]))
    assert d["n_gpus"] == 1 and d["metric"].startswith("time-steps/sec") and d["higher_is_better"] is True
    # per-solve HIP-event durations and their median beside the contract's wall clock
    m = d["median"]
    assert m["reps"] == 3 and m["min_ms"] <= m["ms_per_step"] <= m["max_ms"] and m["value"] == pytest.approx(
        d["config"]["time_steps"] / (m["ms_per_step"] / 1e3), rel=1e-9)
    assert m["min_ms"] * 3 <= d["ms_per_step"] * 3 * 1.0001
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1.5
    assert r["traffic"] is None or (r["traffic"] > 0 and r["traffic_measured"]["launches"] > 0 and "MEASURED" in r["traffic_note"])
    if r["traffic"] is None:
        assert "not measured" in r["traffic_note"]
    assert r["rocprofv3"] is None or r["rocprofv3"]["us_per_time_step"] > 0
    if config == "c5":
        # round 5: the capturable IMEX configuration (direct solves, ksponly) is covered by the default launch mode
        assert d["config"]["launch_mode"] == "graph(auto)", d["config"]["launch_mode"]
    if config == "c3a":
        # the measured streaming ceiling, every kernel on its own moved bytes, the figures beside `frac`
        c = r["copy_ceiling"]
        assert c is not None and c["unit"] == "GB/s" and c["memcpy_d2d_256MiB_GBps"] > 1000
        for key in ("large_stream", "state_size_cold", "state_size_behind_gemm", "state_size_hot"):
            assert 1 < c[key]["GBps"] < 4 * 8000 and c[key]["launches"] >= 10, key      # (64 KiB vectors here: launch-bound)
        assert c["large_stream"]["GBps"] > 2000
        assert c["large_stream"]["bytes_per_launch"] == 3 * (256 << 20) and c["state_size_cold"]["bytes_per_launch"] == 3 * 256 * 64 * 4
        head = r["rocprofv3"] or r["hip_events"]
        fr = [v["frac"] for k, v in head["per_kernel"].items() if "frac" in v]
        assert fr and all(0 < x < 4 for x in fr)
        assert 0 < r["frac_state_vectors"] < 1.5 and 0 < r["frac_moved"] < 1.5 and r["dominant_kernel"]["frac"] > 0
        assert r["dominant_kernel"]["frac_of_copy_ceiling"] > 0 and r["frac_of_copy_ceiling"] > 0
        # round 5: the Linear layers' sensitivities are formed by the engine (no separate accumulation pass, hence no SURVEY credit
        # to flag); the old path is a variant of the same line
        assert d["config"]["linear_param_grads"].startswith("engine (8 of 8") and r["credits"] == []
        # ... by the fused dW + db MFMA kernel at these shapes (256 rows, 64 features), priced on the fp32 MFMA roofline; the
        # library GEMM + bias-sum pass it replaces is a variant as well
        assert "fused dW + db MFMA kernel on 4 layers" in d["config"]["linear_param_grads"]
        lw = r["linear_wgrad"]
        # (fp32 states: operands split into three bf16 terms, six bf16 MFMA products per fp32 product -- the ALGORITHMIC fp32 FLOPs are
        # priced on the fp32 matrix peak, what the bf16 pipe executes on the bf16 peak)
        assert lw["bound"] == "mfma" and lw["unit"] == "TFLOP/s" and lw["peak"] == 157.3 and 0 < lw["frac"] < 16 / 6
        assert lw["kernel"].endswith("x3") and "three bf16 terms" in lw["arithmetic"]
        mp = lw["matrix_pipe"]
        assert mp["peak"] == 2500.0 and mp["achieved"] == pytest.approx(6 * lw["achieved"]) and 0 < mp["frac"] < 1
        assert lw["achieved"] == pytest.approx(lw["flops_per_launch"] / (lw["avg_us"] * 1e-6) / 1e12, rel=1e-6)
        # grouped launches (round 6): the four layers of a stage VJP in ONE launch, four stage VJPs per rk4 time step
        assert lw["flops_per_launch"] == 4 * 2 * 256 * 64 * 64 and lw["launches_per_time_step"] == 4
        assert lw["pairs_per_launch"] == 4.0 and lw["us_per_pair"] == pytest.approx(lw["avg_us"] / 4)
        assert not any(k.startswith("pn_colsum_partial_kernel") for k in head["per_kernel"])
        assert r["hip_events"]["per_kernel"]["pn_linear_wgrad"]["launches"] > 0
        assert d["variants"]["autograd-param-grads"]["value"] > 0 and d["variants"]["library-gemm-param-grads"]["value"] > 0
        assert d["variants"]["fp32-mfma-param-grads"]["value"] > 0 and d["variants"]["side-stream"]["value"] > 0
        assert r["frac_traffic"] is None or r["frac_traffic"] > 0
        v = d["variants"]["f64"]
        assert v["dtype"] == "f64" and v["value"] > 0
        assert "roofline" not in v or 0 < v["roofline"]["frac"] < 1.5


def test_bench_plain_run_times_the_headline_only_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline alone (no roofline pass, profiler children, variants or CPU baseline);
    --dump-outputs writes what the last timed solve returned, the same arrays on a second run with the same arguments."""
    import numpy as np
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "256", "--dim", "64", "--nt", "6"]
    runs = []
    for i in range(2):
        d = _run_bench(argv + ["--dump-outputs", str(tmp_path / str(i))])
        assert d["steps"] == 3 and d["median"]["reps"] == 3 and d["dtype"] == "f32" and d["unit"] == "time-steps/s"
        assert d["value"] == pytest.approx(6 * 3 / (d["ms_per_step"] * 3 / 1e3), rel=1e-6)
        assert d["roofline"] is None and d["variants"] is None and d["cpu_baseline"] is None
        runs.append({f: np.load(str(tmp_path / str(i) / f)) for f in os.listdir(str(tmp_path / str(i)))})
    a, b = runs
    assert sorted(a) == sorted(b) and {"out.npy", "dy0.npy", "loss.npy"} <= set(a) and len(a) == 3 + 8
    assert a["out.npy"].shape == (1, 256, 64) and a["dy0.npy"].shape == (256, 64) and a["out.npy"].dtype == np.float32
    for f in a:
        assert np.all(np.isfinite(a[f])) and np.allclose(a[f], b[f], rtol=1e-6, atol=0), f


def test_bench_config_c3b_stiff_line():
    """bench.py --config c3b --stiff through the same contract: the adaptive workload that adapts -- more
    than 100 accepted steps, rejections, eager launches, a roofline over the error-norm kernel's launches."""
    import json
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PN_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c3b", "--stiff", "--steps", "1", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-variants", "--no-rocprof", "--no-pmc"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["workload"].startswith("C3b --stiff") and d["config"]["launch_mode"].startswith(("graph(auto; per-evaluation", "eager"))
    assert d["config"]["time_steps"] > 100 and d["config"]["rejected_attempts"] >= 5
    assert d["value"] == pytest.approx(d["config"]["time_steps"] / (d["ms_per_step"] / 1e3), rel=1e-6)
    pk = d["roofline"]["hip_events"]["per_kernel"]
    assert pk["pn_rk_combine_wrms"]["launches"] >= d["config"]["time_steps"] + d["config"]["rejected_attempts"]
    assert 0.3 < d["roofline"]["frac"] < 1.0 and d["roofline"]["bound"] == "hbm" and d["roofline"]["traffic"] is None


def test_bench_eight_ranks_sharing_the_device_shards_concatenate_to_the_one_rank_answer(tmp_path):
    """the 8-rank flow of bench.py before an 8-GPU node ever runs it.  Under the driver's N > 1 launch line
    with eight ranks sharing this box's GPU (PN_BENCH_BACKEND=gloo): c3a (fixed-step rk4, graphs captured per rank, ONE
    all-reduce of dL/dtheta per backward), c4 --strong with BASELINE config 4's global batch of 1024 split 128 per rank (reduced
    spatial size) and c3b (adaptive: one 2-double all-reduce per step attempt).  One JSON line each, n_gpus 8, the collectives
    timed, the same step count on every rank -- and the states / dL/dy0 of the eight shards concatenate to, dL/dtheta sums to,
    what ONE rank computes on the whole batch.  Partitioning: SURVEY 8(e); the reference is single-process (pa.py:367)."""
    import json
    import subprocess
    if not torch.cuda.is_available():
        pytest.skip("no HIP device in this container")
    common = ["--steps", "2", "--warmup", "1", "--strong", "--full", "--no-cpu-baseline", "--no-variants", "--no-rocprof", "--no-pmc", "--no-ceiling"]
    cases = {"c3a": ["--config", "c3a", "--batch", "512", "--dim", "64", "--nt", "6"],
             "c4": ["--config", "c4", "--batch", "1024", "--hw", "4", "--nt", "2"],
             "c3b": ["--config", "c3b", "--batch", "512", "--dim", "32"]}
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = {}
    for name, argv in cases.items():
        # one configuration at a time (its 8-rank and its 1-rank run side by side): the launch mode `auto` settles on is decided
        # by the clock -- replay must not be slower than the eager launches -- and 27 processes on one device blur it
        procs = {}
        for world in (8, 1):
            dump = str(tmp_path / ("%s_%d.pt" % (name, world)))
            launcher = (["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                         "--master-port", str(_free_port())] if world > 1 else [])
            cmd = [sys.executable] + launcher + [os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--dump", dump] + common + argv
            procs[(name, world)] = (subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                                                     env=dict(env, PN_BENCH_BACKEND="gloo", OMP_NUM_THREADS="2")), dump)
        for key, (p, dump) in procs.items():
            so, se = p.communicate(timeout=600)
            assert p.returncode == 0, (key, so[-1500:], se[-3000:])
            lines = [l for l in so.splitlines() if l.startswith("{")]
            assert len(lines) == 1, (key, so)
            res[key] = (json.loads(lines[0]), torch.load(dump))
    for name in cases:
        d8, s8 = res[(name, 8)]
        d1, s1 = res[(name, 1)]
        assert d8["n_gpus"] == 8 and d8["scaling"] == "strong" and d1["n_gpus"] == 1
        assert d8["config"]["allreduce_us"] > 0 and len(d8["config"]["time_steps_per_rank"]) == 8
        assert len(set(d8["config"]["time_steps_per_rank"])) == 1 and s8["steps_per_rank"] == d8["config"]["time_steps_per_rank"]
        assert d8["config"]["time_steps"] == d1["config"]["time_steps"]
        assert d8["value"] == pytest.approx(8 * d8["config"]["time_steps"] * 2 / (d8["ms_per_step"] * 2 / 1e3), rel=1e-6)
        if name == "c3b":
            assert d8["config"]["enorm_allreduce_us"] > 0 and d8["config"]["launch_mode"].startswith("eager") and d8["config"]["time_steps"] >= 2
        else:
            # (the launch mode `auto` settles on is decided by the clock -- replay must not be slower than the eager launches -- and
            # nine processes share this device: "graph(auto)" on a quiet box, eager launches with the reason otherwise; what this
            # test is about, the shards against the one-rank answer, holds either way)
            assert d8["config"]["enorm_allreduce_us"] is None and d8["config"]["launch_mode"].startswith(("graph", "eager"))
        # fp32: the GEMM / MIOpen convolution kernels PyTorch picks depend on the rows per rank (c4's dL/dy0 is O(1e-6) per
        # element and came out 3.5e-5 apart); the adaptive c3b adds the summation order of the global error norm
        tol = {"c3a": 2e-5, "c4": 2e-4, "c3b": 1e-4}[name]
        assert s8["out"].shape == s1["out"].shape and s8["dy0"].shape == s1["dy0"].shape
        assert _rel(s8["out"], s1["out"]) < tol and _rel(s8["dy0"], s1["dy0"]) < tol and _rel(s8["dtheta"], s1["dtheta"]) < 5 * tol, name


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
