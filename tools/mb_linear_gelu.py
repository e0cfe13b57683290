"""Times what -pn_linear_gelu 1 puts in place of torch for an nn.Linear -> nn.GELU pair of func, on the same operands in one process:
     forward, y alone   pn_linear_fwd with PN_ACT_GELU         against  F.linear(x, w, b) + gelu
     forward, y and z   pn_linear_fwd_pre with PN_ACT_GELU     against  the same (the stock pair saves its pre-activation anyway)
     backward           pn_linear_bwd_act with PN_ACT_GELU     against  gelu_backward + matmul(g_z, w)        (the stock modules)
                                                               and      gelu_backward + pn_linear_dx(g_z, w)  (what -pn_linear_bare 1 runs)
(csrc/pn_linear.hip).  Every side is captured into a hipGraph of N launches (or launch pairs) and replayed: no Python between two
launches, the way a graph-mode sweep runs them.  pn_linear_fwd with the identity, tanh and sigmoid and pn_linear_bwd (tanh) are timed
beside them, in interleaved rounds: round r times one block of every graph in turn, so that a drift of the clocks falls on all of them
alike (the method of tools/mb_linear_sigmoid.py).
     python tools/mb_linear_gelu.py                      every shape below, each in a fresh child process
     python tools/mb_linear_gelu.py rows out_f in_f      one shape, in this process
Prints the median and the fastest block in us per launch (per launch pair); how far y is from float64 GELU of the identity forward and
g_z from g d64(z), each beside the stock fp32 operation's own error on the same operands, in units of 2^-24; that z is the identity
forward's y, y the y-only form's and dx pn_linear_dx's of g_z bit for bit; and the errors against float64 end to end."""
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

    def gb(g, z):
        return torch.ops.aten.gelu_backward(g, z, approximate="none")
    gs = [torch.randn(rows, out_f, device=dev) for _ in range(NP)]
    xs = [torch.randn(rows, in_f, device=dev) for _ in range(NP)]
    ws = [torch.randn(out_f, in_f, device=dev) / out_f ** 0.5 for _ in range(NP)]
    bs = [torch.randn(out_f, device=dev) for _ in range(NP)]
    pres = [torch.randn(rows, out_f, device=dev) for _ in range(NP)]                   # a pair's pre-activation
    tanhs = [torch.tanh(torch.randn(rows, out_f, device=dev)) for _ in range(NP)]
    gzs = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    dxs = [torch.empty(rows, in_f, device=dev) for _ in range(NP)]
    ys = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    zs = [torch.empty(rows, out_f, device=dev) for _ in range(NP)]
    ops = HipVecOps(dev, torch.float32, rows * max(out_f, in_f))
    assert ops.linear_bwd_supported(rows, out_f, in_f) and ops.linear_fwd_supported(rows, out_f, in_f)

    def each(fn):
        def run():
            for k in range(N):
                fn(k % NP)
        return run

    sides = (
        ("pn_linear_fwd gelu (y)", each(lambda i: ops.linear_act_fwd(xs[i], ws[i], bs[i], "gelu", ys[i], flags=0))),
        ("pn_linear_fwd_pre gelu (y, z)", each(lambda i: ops.linear_act_fwd(xs[i], ws[i], bs[i], "gelu", ys[i], zs[i], flags=0))),
        ("pn_linear_fwd sigmoid", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0, act="sigmoid"))),
        ("pn_linear_fwd tanh", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], True, ys[i], flags=0))),
        ("pn_linear_fwd identity", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0))),
        ("F.linear + gelu", each(lambda i: F.gelu(F.linear(xs[i], ws[i], bs[i])))),
        ("pn_linear_bwd_act gelu", each(lambda i: ops.linear_bwd(gs[i], pres[i], ws[i], gzs[i], dxs[i], flags=0, act="gelu"))),
        ("pn_linear_bwd (tanh)", each(lambda i: ops.linear_bwd(gs[i], tanhs[i], ws[i], gzs[i], dxs[i], flags=0))),
        ("gelu_bwd + matmul", each(lambda i: torch.matmul(gb(gs[i], pres[i]), ws[i], out=dxs[i]))),
        ("gelu_bwd + pn_linear_dx", each(lambda i: ops.linear_dx(gb(gs[i], pres[i]), ws[i], dxs[i], flags=0))),
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
        print("%-30s %4d x %4d x %4d: median %6.2f us (fastest %6.2f) per launch" % (name, rows, out_f, in_f, med, best))
    U = 2.0 ** 24
    g, x, w, b, pre = gs[0], xs[0], ws[0], bs[0], pres[0]
    z = torch.empty(rows, out_f, device=dev)
    y = ops.linear_act_fwd(x, w, b, "gelu", z=z)
    ident = ops.linear_fwd(x, w, b, False)
    print("z is the identity forward's y bit for bit: %s;  y is the y-only form's: %s" % (
        torch.equal(z.view(torch.int32), ident.view(torch.int32)),
        torch.equal(y.view(torch.int32), ops.linear_act_fwd(x, w, b, "gelu").view(torch.int32))))

    def gelu64(v):
        v = v.double()
        return 0.5 * v * (1.0 + torch.erf(v * 0.5 ** 0.5))

    def d64(v):
        v = v.double()
        return 0.5 * (1.0 + torch.erf(v * 0.5 ** 0.5)) + v * torch.exp(-0.5 * v * v) * (2.0 * torch.pi) ** -0.5
    ref = gelu64(ident)
    print("forward:  max |y - gelu64(z)| = %.2f x 2^-24 (F.gelu(z): %.2f);  over max(1, |z|): %.2f (F.gelu: %.2f)" % (
        float((y.double() - ref).abs().max()) * U, float((F.gelu(ident).double() - ref).abs().max()) * U,
        float(((y.double() - ref).abs() / ident.double().abs().clamp(min=1)).max()) * U,
        float(((F.gelu(ident).double() - ref).abs() / ident.double().abs().clamp(min=1)).max()) * U))
    gz, dx = ops.linear_bwd(g, pre, w, act="gelu")
    gz_t = gb(g, pre)
    gz64 = g.double() * d64(pre)
    print("backward: max |g_z - g d64(z)| / |g| = %.2f x 2^-24 (gelu_backward: %.2f), dx pn_linear_dx's of g_z bit for bit: %s" % (
        float(((gz.double() - gz64).abs() / g.double().abs()).max()) * U, float(((gz_t.double() - gz64).abs() / g.double().abs()).max()) * U,
        torch.equal(dx.view(torch.int32), ops.linear_dx(gz, w).view(torch.int32))))
    ref = gelu64(x.double() @ w.double().t() + b.double())
    scale = x.double().abs() @ w.double().abs().t() + b.double().abs()
    print("y:  max |err| / (|x| @ |w|^T + |b|):  pn_linear_fwd_pre gelu %.3e   library %.3e" % (
        float(((y.double() - ref).abs() / scale).max()), float(((F.gelu(F.linear(x, w, b)).double() - ref).abs() / scale).max())))
    ref = gz64 @ w.double()
    scale = gz64.abs() @ w.double().abs()
    ok = scale > 0
    print("dx: max |err| / (|g_z| @ |w|):  pn_linear_bwd_act gelu %.3e   library %.3e" % (
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
