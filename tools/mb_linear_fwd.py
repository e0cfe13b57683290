"""Times pn_linear_fwd (csrc/pn_linear.hip) against the library path it replaces, torch.tanh(F.linear(x, w, b)), on the same
operands in one process.  Both sides are captured into hipGraphs of N launches and replayed: no Python between two launches, the
way a graph-mode sweep runs them.     python tools/mb_linear_fwd.py [rows out_f in_f]
Both forms of the kernel's K loop (the pipelined one and PN_LINEAR_FORM_PLAIN) are timed in the same process, in interleaved rounds: round r
times one block of every graph in turn, so that a drift of the clocks falls on all of them alike.
Prints the median and the fastest block in us per launch (the library side: per pair of launches) and the error against float64."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

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
    xs = [torch.randn(rows, in_f, device=dev) for _ in range(NP)]
    ws = [torch.randn(out_f, in_f, device=dev) / in_f ** 0.5 for _ in range(NP)]
    bs = [torch.randn(out_f, device=dev) for _ in range(NP)]
    ys = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    ops = HipVecOps(dev, torch.float32, rows * in_f)
    assert ops.linear_fwd_supported(rows, out_f, in_f)

    def ours(tanh, flags=0):
        for k in range(N):
            ops.linear_fwd(xs[k % NP], ws[k % NP], bs[k % NP], tanh, ys[k % NP], flags=flags)

    def plain(tanh):
        ours(tanh, _lib.PN_LINEAR_FORM_PLAIN)

    def lib(tanh):
        for k in range(N):
            z = F.linear(xs[k % NP], ws[k % NP], bs[k % NP])
            if tanh:
                torch.tanh(z)

    side = torch.cuda.Stream()
    graphs = {}
    for name, fn, arg in (("pn_linear_fwd tanh pipelined", ours, True), ("pn_linear_fwd tanh plain", plain, True),
                          ("pn_linear_fwd identity pipelined", ours, False), ("pn_linear_fwd identity plain", plain, False),
                          ("torch.tanh(F.linear)", lib, True), ("F.linear", lib, False)):
        with torch.cuda.stream(side):
            fn(arg)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn(arg)
        torch.cuda.synchronize()
        graphs[name] = g
    results = timed(graphs, N)
    for name, (med, best) in results.items():
        print("%-32s %4d x %4d x %4d: median %6.2f us (fastest %6.2f) per layer evaluation" % (name, rows, out_f, in_f, med, best))
    x, w, b = xs[0], ws[0], bs[0]
    z64 = F.linear(x.double(), w.double(), b.double())
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    for tanh in (False, True):
        ref = torch.tanh(z64) if tanh else z64
        got = ops.linear_fwd(x, w, b, tanh)
        print("act=%s  the two forms give the same bits: %s" % (
            "tanh" if tanh else "identity", torch.equal(got, ops.linear_fwd(x, w, b, tanh, flags=_lib.PN_LINEAR_FORM_PLAIN))))
        libv = torch.tanh(F.linear(x, w, b)) if tanh else F.linear(x, w, b)
        print("act=%s  max error / (sum|x w| + |b|):  pn_linear_fwd %.3e   library %.3e" % (
            "tanh" if tanh else "identity", float(((got.double() - ref).abs() / scale).max()), float(((libv.double() - ref).abs() / scale).max())))


if __name__ == "__main__":
    main()
