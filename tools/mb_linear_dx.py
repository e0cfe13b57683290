"""Times what -pn_linear_bare 1 puts in place of the library for a bare nn.Linear of func, on the same operands in one process:
pn_linear_dx (csrc/pn_linear.hip) against torch.matmul(g, w), and pn_linear_fwd with the identity against F.linear(x, w, b).
Every side is captured into a hipGraph of N launches and replayed: no Python between two launches, the way a graph-mode sweep runs them.
     python tools/mb_linear_dx.py [rows out_f in_f]
Both forms of the K loop (pipelined, PN_LINEAR_FORM_PLAIN) and pn_linear_bwd on the same g (with an a of zeros: the kernel pn_linear_dx is
cut from) are timed beside them, in interleaved rounds: round r times one block of every graph in turn, so that a drift of the clocks
falls on all of them alike.  Prints the median and the fastest block in us per launch, that pn_linear_dx has the bits of pn_linear_bwd fed
zeros, and the errors against float64."""
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
    PLAIN = _lib.PN_LINEAR_FORM_PLAIN
    gs = [torch.randn(rows, out_f, device=dev) for _ in range(NP)]
    xs = [torch.randn(rows, in_f, device=dev) for _ in range(NP)]
    zeros = [torch.zeros(rows, out_f, device=dev) for _ in range(NP)]
    ws = [torch.randn(out_f, in_f, device=dev) / out_f ** 0.5 for _ in range(NP)]
    bs = [torch.randn(out_f, device=dev) for _ in range(NP)]
    gzs = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    dxs = [torch.empty(rows, in_f, device=dev) for _ in range(NP)]
    ys = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    ops = HipVecOps(dev, torch.float32, rows * max(out_f, in_f))
    assert ops.linear_dx_supported(rows, out_f, in_f) and ops.linear_fwd_supported(rows, out_f, in_f)

    def each(fn):
        def run():
            for k in range(N):
                fn(k % NP)
        return run

    sides = (
        ("pn_linear_dx pipelined", each(lambda i: ops.linear_dx(gs[i], ws[i], dxs[i], flags=0))),
        ("pn_linear_dx plain", each(lambda i: ops.linear_dx(gs[i], ws[i], dxs[i], flags=PLAIN))),
        ("matmul(g, w)", each(lambda i: torch.matmul(gs[i], ws[i], out=dxs[i]))),
        ("pn_linear_bwd (a = 0)", each(lambda i: ops.linear_bwd(gs[i], zeros[i], ws[i], gzs[i], dxs[i], flags=0))),
        ("pn_linear_fwd identity", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0))),
        ("pn_linear_fwd id. plain", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=PLAIN))),
        ("F.linear(x, w, b)", each(lambda i: F.linear(xs[i], ws[i], bs[i]))),
    )
    side = torch.cuda.Stream()
    graphs = {}
    with torch.no_grad():
        for name, fn in sides:
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
        print("%-24s %4d x %4d x %4d: median %6.2f us (fastest %6.2f) per launch" % (name, rows, out_f, in_f, med, best))
    g, x, w, b = gs[0], xs[0], ws[0], bs[0]
    dx, dx_p = ops.linear_dx(g, w), ops.linear_dx(g, w, flags=PLAIN)
    _, dx_b = ops.linear_bwd(g, zeros[0], w)
    print("pn_linear_dx: the two forms give the same bits: %s; the bits of pn_linear_bwd fed zeros: %s" % (torch.equal(dx, dx_p), torch.equal(dx, dx_b)))
    ref = g.double() @ w.double()
    scale = g.double().abs() @ w.double().abs()
    print("dx: max |err| / (|g| @ |w|):  pn_linear_dx %.3e   library %.3e" % (
        float(((dx.double() - ref).abs() / scale).max()), float(((torch.matmul(g, w).double() - ref).abs() / scale).max())))
    y = ops.linear_fwd(x, w, b, False)
    ref = x.double() @ w.double().t() + b.double()
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    print("y:  max |err| / (|x| @ |w|^T + |b|):  pn_linear_fwd %.3e   library %.3e" % (
        float(((y.double() - ref).abs() / scale).max()), float(((F.linear(x, w, b).double() - ref).abs() / scale).max())))


if __name__ == "__main__":
    main()
