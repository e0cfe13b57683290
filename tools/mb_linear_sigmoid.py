"""Times what -pn_linear_sigmoid 1 puts in place of torch for an nn.Linear -> nn.Sigmoid pair of func, on the same operands in one process:
     forward   pn_linear_fwd with PN_ACT_SIGMOID          against  F.linear(x, w, b) + sigmoid
     backward  pn_linear_bwd_act with PN_ACT_SIGMOID      against  sigmoid_backward + matmul(g_z, w)        (the stock modules)
                                                          and      sigmoid_backward + pn_linear_dx(g_z, w)  (what -pn_linear_bare 1 runs)
(csrc/pn_linear.hip).  Every side is captured into a hipGraph of N launches (or launch pairs) and replayed: no Python between two
launches, the way a graph-mode sweep runs them.  pn_linear_fwd with the identity and pn_linear_bwd (tanh) are timed beside them, in
interleaved rounds: round r times one block of every graph in turn, so that a drift of the clocks falls on all of them alike.
     python tools/mb_linear_sigmoid.py                      every shape below, each in a fresh child process
     python tools/mb_linear_sigmoid.py rows out_f in_f      one shape, in this process
Prints the median and the fastest block in us per launch (per launch pair), how far the Sigmoid forward is from sigma of the identity
forward and g_z from g a (1 - a) in units of 2^-24, that dx is pn_linear_dx's of g_z bit for bit, and the errors against float64."""
import os
import subprocess
import sys

SHAPES = [(4096, 512, 512)]        # the headline's


def timed(graphs, n, reps=20, rounds=9):
    """{name: graph} -> {name: (median, fastest)} us per launch; one block = reps replays, the graphs take turns inside a round"""
    import torch
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


def one_shape(rows, out_f, in_f):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.nn.functional as F

    import pnode_amd  # noqa: F401
    from pnode_amd._vecops import HipVecOps
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    NP, N = 4, 48
    sb = torch.ops.aten.sigmoid_backward
    gs = [torch.randn(rows, out_f, device=dev) for _ in range(NP)]
    xs = [torch.randn(rows, in_f, device=dev) for _ in range(NP)]
    ws = [torch.randn(out_f, in_f, device=dev) / out_f ** 0.5 for _ in range(NP)]
    bs = [torch.randn(out_f, device=dev) for _ in range(NP)]
    acts = [torch.sigmoid(torch.randn(rows, out_f, device=dev)) for _ in range(NP)]    # a pair's output
    tanhs = [torch.tanh(torch.randn(rows, out_f, device=dev)) for _ in range(NP)]
    gzs = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    dxs = [torch.empty(rows, in_f, device=dev) for _ in range(NP)]
    ys = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    ops = HipVecOps(dev, torch.float32, rows * max(out_f, in_f))
    assert ops.linear_bwd_supported(rows, out_f, in_f) and ops.linear_fwd_supported(rows, out_f, in_f)

    def each(fn):
        def run():
            for k in range(N):
                fn(k % NP)
        return run

    sides = (
        ("pn_linear_fwd sigmoid", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0, act="sigmoid"))),
        ("pn_linear_fwd tanh", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], True, ys[i], flags=0))),
        ("pn_linear_fwd identity", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0))),
        ("F.linear + sigmoid", each(lambda i: torch.sigmoid(F.linear(xs[i], ws[i], bs[i])))),
        ("pn_linear_bwd_act sigmoid", each(lambda i: ops.linear_bwd(gs[i], acts[i], ws[i], gzs[i], dxs[i], flags=0, act="sigmoid"))),
        ("pn_linear_bwd (tanh)", each(lambda i: ops.linear_bwd(gs[i], tanhs[i], ws[i], gzs[i], dxs[i], flags=0))),
        ("sigmoid_bwd + matmul", each(lambda i: torch.matmul(sb(gs[i], acts[i]), ws[i], out=dxs[i]))),
        ("sigmoid_bwd + pn_linear_dx", each(lambda i: ops.linear_dx(sb(gs[i], acts[i]), ws[i], dxs[i], flags=0))),
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
        print("%-28s %4d x %4d x %4d: median %6.2f us (fastest %6.2f) per launch" % (name, rows, out_f, in_f, med, best))
    g, x, w, b, a = gs[0], xs[0], ws[0], bs[0], acts[0]
    y, ident = ops.linear_fwd(x, w, b, False, act="sigmoid"), ops.linear_fwd(x, w, b, False)
    gz, dx = ops.linear_bwd(g, a, w, act="sigmoid")
    gz_t = sb(g, a)
    gz64 = g.double() * a.double() * (1.0 - a.double())
    print("forward: max |y - sigma(identity forward)| = %.2f x 2^-24;  backward: max |g_z - g a (1 - a)| / |g a (1 - a)| = %.2f x 2^-24 "
          "(sigmoid_backward: %.2f), dx pn_linear_dx's of g_z bit for bit: %s" % (
              float((y.double() - torch.sigmoid(ident.double())).abs().max()) * 2.0 ** 24,
              float(((gz.double() - gz64).abs() / gz64.abs()).max()) * 2.0 ** 24, float(((gz_t.double() - gz64).abs() / gz64.abs()).max()) * 2.0 ** 24,
              torch.equal(dx.view(torch.int32), ops.linear_dx(gz, w).view(torch.int32))))
    ref = torch.sigmoid(x.double() @ w.double().t() + b.double())
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    print("y:  max |err| / (|x| @ |w|^T + |b|):  pn_linear_fwd sigmoid %.3e   library %.3e" % (
        float(((y.double() - ref).abs() / scale).max()), float(((torch.sigmoid(F.linear(x, w, b)).double() - ref).abs() / scale).max())))
    ref = gz64 @ w.double()
    scale = gz64.abs() @ w.double().abs()
    ok = scale > 0
    print("dx: max |err| / (|g_z| @ |w|):  pn_linear_bwd_act sigmoid %.3e   library %.3e" % (
        float(((dx.double() - ref).abs()[ok] / scale[ok]).max()), float(((torch.matmul(gz_t, w).double() - ref).abs()[ok] / scale[ok]).max())))


def main():
    if len(sys.argv) >= 4:
        return one_shape(*(int(v) for v in sys.argv[1:4]))
    # a fresh child process per shape (this one never touches the device): no allocator state, library choice or clock history is shared
    for shape in SHAPES:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(v) for v in shape]).returncode
        if rc != 0:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
