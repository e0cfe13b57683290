"""Times pn_linear_bwd (csrc/pn_linear.hip) against the pair of torch operations it replaces, aten.tanh_backward(g, a) and
torch.matmul(g_z, w), on the same operands in one process.  Both sides are captured into hipGraphs of N launches and replayed: no
Python between two launches, the way a graph-mode sweep runs them.     python tools/mb_linear_bwd.py [rows out_f in_f]
Both forms of the kernel's K loop (the pipelined one and PN_LINEAR_FORM_PLAIN) are timed in the same process, in interleaved rounds: round r
times one block of every graph in turn, so that a drift of the clocks falls on all of them alike.
Prints the median and the fastest block in us per pair backward (the library side: per pair of launches) and the error against float64."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import pnode_amd  # noqa: F401
from pnode_amd import _lib
from pnode_amd._vecops import HipVecOps


def timed(graphs, n, reps=20, rounds=9):
    """{name: graph} -> {name: (median, fastest)} us per launch; one block = reps replays, the graphs take turns inside a round"""
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            e0.record()
            for _ in range(reps):
                g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / (reps * n))
    return {name: (sorted(t)[len(t) // 2], min(t)) for name, t in times.items()}


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

    def ours(flags):
        for k in range(N):
            ops.linear_bwd(gs[k % NP], acts[k % NP], ws[k % NP], gzs[k % NP], dxs[k % NP], flags=flags)

    def lib():
        for k in range(N):
            torch.matmul(torch.ops.aten.tanh_backward(gs[k % NP], acts[k % NP]), ws[k % NP])

    def lib_matmul():
        for k in range(N):
            torch.matmul(gs[k % NP], ws[k % NP])

    side = torch.cuda.Stream()
    graphs = {}
    for name, fn in (("pn_linear_bwd pipelined", lambda: ours(0)), ("pn_linear_bwd plain", lambda: ours(_lib.PN_LINEAR_FORM_PLAIN)),
                     ("tanh_backward + matmul", lib), ("matmul alone", lib_matmul)):
        with torch.cuda.stream(side):
            fn()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                fn()
        torch.cuda.synchronize()
        graphs[name] = graph
    results = timed(graphs, N)
    for name, (med, best) in results.items():
        print("%-24s %4d x %4d x %4d: median %6.2f us (fastest %6.2f) per pair backward" % (name, rows, out_f, in_f, med, best))
    g, a, w = gs[0], acts[0], ws[0]
    gz64 = g.double() * (1.0 - a.double() * a.double())
    gz, dx = ops.linear_bwd(g, a, w)
    gz_p, dx_p = ops.linear_bwd(g, a, w, flags=_lib.PN_LINEAR_FORM_PLAIN)
    print("the two forms give the same bits: gz %s, dx %s" % (torch.equal(gz, gz_p), torch.equal(dx, dx_p)))
    gz_lib = torch.ops.aten.tanh_backward(g, a)
    print("g_z: max |err| / |g|:  pn_linear_bwd %.3e   library %.3e   (3 * 2^-24 = %.3e)" % (
        float(((gz.double() - gz64).abs() / g.double().abs()).max()), float(((gz_lib.double() - gz64).abs() / g.double().abs()).max()), 3.0 * 2.0 ** -24))
    ref = gz.double() @ w.double()
    scale = gz.double().abs() @ w.double().abs()
    print("dx on pn_linear_bwd's g_z: max |err| / (|g_z| @ |w|):  pn_linear_bwd %.3e   library %.3e" % (
        float(((dx.double() - ref).abs() / scale).max()), float(((torch.matmul(gz, w).double() - ref).abs() / scale).max())))


if __name__ == "__main__":
    main()
