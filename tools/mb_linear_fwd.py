"""Times pn_linear_fwd (csrc/pn_linear.hip) against the library path it replaces, torch.tanh(F.linear(x, w, b)), on the same
operands in one process.  Both sides are captured into hipGraphs of N launches and replayed: no Python between two launches, the
way a graph-mode sweep runs them.     python tools/mb_linear_fwd.py [rows out_f in_f]
Prints us per launch (the library side: per pair of launches) and the error of both against float64."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import pnode_amd  # noqa: F401
from pnode_amd._vecops import HipVecOps


def timed(graph, n, reps=20):
    for _ in range(3):
        graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            graph.replay()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / (reps * n))
    return best


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

    def ours(tanh):
        for k in range(N):
            ops.linear_fwd(xs[k % NP], ws[k % NP], bs[k % NP], tanh, ys[k % NP])

    def lib(tanh):
        for k in range(N):
            z = F.linear(xs[k % NP], ws[k % NP], bs[k % NP])
            if tanh:
                torch.tanh(z)

    side = torch.cuda.Stream()
    results = {}
    for name, fn, arg in (("pn_linear_fwd tanh", ours, True), ("pn_linear_fwd identity", ours, False),
                          ("torch.tanh(F.linear)", lib, True), ("F.linear", lib, False)):
        with torch.cuda.stream(side):
            fn(arg)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn(arg)
        torch.cuda.synchronize()
        results[name] = timed(g, N)
    for name in results:
        print("%-24s %4d x %4d x %4d: %6.2f us per layer evaluation" % (name, rows, out_f, in_f, results[name]))
    x, w, b = xs[0], ws[0], bs[0]
    z64 = F.linear(x.double(), w.double(), b.double())
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    for tanh in (False, True):
        ref = torch.tanh(z64) if tanh else z64
        got = ops.linear_fwd(x, w, b, tanh)
        libv = torch.tanh(F.linear(x, w, b)) if tanh else F.linear(x, w, b)
        print("act=%s  max error / (sum|x w| + |b|):  pn_linear_fwd %.3e   library %.3e" % (
            "tanh" if tanh else "identity", float(((got.double() - ref).abs() / scale).max()), float(((libv.double() - ref).abs() / scale).max())))


if __name__ == "__main__":
    main()
