"""Times what -pn_linear_relu 1 puts in place of torch for an nn.Linear -> nn.ReLU pair of func, on the same operands in one process:
     forward   pn_linear_fwd with PN_ACT_RELU             against  F.linear(x, w, b) + relu
     backward  pn_linear_bwd_act with PN_ACT_RELU         against  threshold_backward + matmul(g_z, w)        (the stock modules)
                                                          and      threshold_backward + pn_linear_dx(g_z, w)  (what -pn_linear_bare 1 runs)
(csrc/pn_linear.hip).  Every side is captured into a hipGraph of N launches (or launch pairs) and replayed: no Python between two
launches, the way a graph-mode sweep runs them.  pn_linear_fwd with the identity and pn_linear_bwd (tanh) are timed beside them, in
interleaved rounds: round r times one block of every graph in turn, so that a drift of the clocks falls on all of them alike.
     python tools/mb_linear_relu.py                      every shape below, each in a fresh child process
     python tools/mb_linear_relu.py rows out_f in_f      one shape, in this process
Prints the median and the fastest block in us per launch (per launch pair), that the ReLU forward is relu of the identity forward, that
g_z is threshold_backward's and dx pn_linear_dx's of it bit for bit, and the errors against float64."""
import os
import subprocess
import sys

SHAPES = [(4096, 512, 512), (4096, 1152, 1152)]        # the headline's; the hidden width of the Burgers net


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
    tb = torch.ops.aten.threshold_backward
    gs = [torch.randn(rows, out_f, device=dev) for _ in range(NP)]
    xs = [torch.randn(rows, in_f, device=dev) for _ in range(NP)]
    ws = [torch.randn(out_f, in_f, device=dev) / out_f ** 0.5 for _ in range(NP)]
    bs = [torch.randn(out_f, device=dev) for _ in range(NP)]
    acts = [torch.relu(torch.randn(rows, out_f, device=dev)) for _ in range(NP)]       # a pair's output: half of it zeros
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
        ("pn_linear_fwd relu", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0, act="relu"))),
        ("pn_linear_fwd identity", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0))),
        ("F.linear + relu", each(lambda i: torch.relu(F.linear(xs[i], ws[i], bs[i])))),
        ("pn_linear_bwd_act relu", each(lambda i: ops.linear_bwd(gs[i], acts[i], ws[i], gzs[i], dxs[i], flags=0, act="relu"))),
        ("pn_linear_bwd (tanh)", each(lambda i: ops.linear_bwd(gs[i], tanhs[i], ws[i], gzs[i], dxs[i], flags=0))),
        ("threshold_bwd + matmul", each(lambda i: torch.matmul(tb(gs[i], acts[i], 0), ws[i], out=dxs[i]))),
        ("threshold_bwd + pn_linear_dx", each(lambda i: ops.linear_dx(tb(gs[i], acts[i], 0), ws[i], dxs[i], flags=0))),
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
    y, ident = ops.linear_fwd(x, w, b, False, act="relu"), ops.linear_fwd(x, w, b, False)
    gz, dx = ops.linear_bwd(g, a, w, act="relu")
    gz_t = tb(g, a, 0)
    print("forward: relu of the identity forward, value for value: %s;  backward: g_z threshold_backward's bits: %s, dx pn_linear_dx's of it: %s" % (
        torch.equal(y, torch.relu(ident)), torch.equal(gz.view(torch.int32), gz_t.view(torch.int32)),
        torch.equal(dx.view(torch.int32), ops.linear_dx(gz, w).view(torch.int32))))
    ref = torch.relu(x.double() @ w.double().t() + b.double())
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    print("y:  max |err| / (|x| @ |w|^T + |b|):  pn_linear_fwd relu %.3e   library %.3e" % (
        float(((y.double() - ref).abs() / scale).max()), float(((torch.relu(F.linear(x, w, b)).double() - ref).abs() / scale).max())))
    ref = gz_t.double() @ w.double()
    scale = gz_t.double().abs() @ w.double().abs()
    ok = scale > 0
    print("dx: max |err| / (|g_z| @ |w|):  pn_linear_bwd_act relu %.3e   library %.3e" % (
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
