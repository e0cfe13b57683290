"""Times pn_linear_bwd (csrc/pn_linear.hip) against the pair of torch operations it replaces, aten.tanh_backward(g, a) and
torch.matmul(g_z, w), on the same operands in one process.  Both sides are captured into hipGraphs of N launches and replayed: no
Python between two launches, the way a graph-mode sweep runs them.     python tools/mb_linear_bwd.py [rows out_f in_f]
Prints the median us per pair backward (the library side: per pair of launches) and the error of both against float64."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pnode_amd  # noqa: F401
from pnode_amd._vecops import HipVecOps


def timed(graph, n, reps=20, rounds=9):
    for _ in range(3):
        graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(rounds):
        e0.record()
        for _ in range(reps):
            graph.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (reps * n))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    rows, out_f, in_f = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (4096, 512, 512)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    NP, N = 4, 48
    gs = [torch.randn(rows, out_f, device=dev) for _ in range(NP)]
    acts = [torch.tanh(torch.randn(rows, out_f, device=dev)) for _ in range(NP)]
    ws = [torch.randn(out_f, in_f, device=dev) / out_f ** 0.5 for _ in range(NP)]
    gzs = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    dxs = [torch.empty(rows, in_f, device=dev) for _ in range(NP)]
    ops = HipVecOps(dev, torch.float32, rows * out_f)
    assert ops.linear_bwd_supported(rows, out_f, in_f)

    def ours():
        for k in range(N):
            ops.linear_bwd(gs[k % NP], acts[k % NP], ws[k % NP], gzs[k % NP], dxs[k % NP])

    def lib():
        for k in range(N):
            torch.matmul(torch.ops.aten.tanh_backward(gs[k % NP], acts[k % NP]), ws[k % NP])

    def lib_matmul():
        for k in range(N):
            torch.matmul(gs[k % NP], ws[k % NP])

    side = torch.cuda.Stream()
    results = {}
    for name, fn in (("pn_linear_bwd", ours), ("tanh_backward + matmul", lib), ("matmul alone", lib_matmul)):
        with torch.cuda.stream(side):
            fn()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                fn()
        torch.cuda.synchronize()
        results[name] = timed(graph, N)
    for name, (med, best) in results.items():
        print("%-24s %4d x %4d x %4d: median %6.2f us (fastest %6.2f) per pair backward" % (name, rows, out_f, in_f, med, best))
    g, a, w = gs[0], acts[0], ws[0]
    gz64 = g.double() * (1.0 - a.double() * a.double())
    gz, dx = ops.linear_bwd(g, a, w)
    gz_lib = torch.ops.aten.tanh_backward(g, a)
    print("g_z: max |err| / |g|:  pn_linear_bwd %.3e   library %.3e   (3 * 2^-24 = %.3e)" % (
        float(((gz.double() - gz64).abs() / g.double().abs()).max()), float(((gz_lib.double() - gz64).abs() / g.double().abs()).max()), 3.0 * 2.0 ** -24))
    ref = gz.double() @ w.double()
    scale = gz.double().abs() @ w.double().abs()
    print("dx on pn_linear_bwd's g_z: max |err| / (|g_z| @ |w|):  pn_linear_bwd %.3e   library %.3e" % (
        float(((dx.double() - ref).abs() / scale).max()), float(((torch.matmul(gz, w).double() - ref).abs() / scale).max())))


if __name__ == "__main__":
    main()
