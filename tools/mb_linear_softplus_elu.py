"""Times what -pn_linear_softplus 1 and -pn_linear_elu 1 put in place of torch for an nn.Linear -> nn.Softplus / nn.ELU pair of func, on the
same operands in one process (the method of tools/mb_linear_sigmoid.py), per act:
     forward   pn_linear_fwd with PN_ACT_SOFTPLUS / PN_ACT_ELU   against  F.linear(x, w, b) + F.softplus / F.elu
     backward  pn_linear_bwd_act with the same act                against  the torch expression + matmul(g_z, w)        (the stock modules)
                                                                  and      the torch expression + pn_linear_dx(g_z, w)  (-pn_linear_bare 1)
the torch expression being g * (-expm1(-a)) for Softplus and aten.elu_backward(g, 1, 1, 1, True, a) for ELU.  Every side is captured
into a hipGraph of N launches (or launch pairs) and replayed; pn_linear_fwd with the identity and the Sigmoid pair's two kernels are timed
beside them, in interleaved rounds.
     python tools/mb_linear_softplus_elu.py                      every shape below, each in a fresh child process
     python tools/mb_linear_softplus_elu.py rows out_f in_f      one shape, in this process
Prints the median and the fastest block in us per launch (per launch pair), the error of y against float64 of the identity forward
relative to |y| and of g_z relative to |g| in units of 2^-24 beside the torch expressions', and that dx is pn_linear_dx's of g_z bit for
bit."""
import os
import subprocess
import sys

from mb_linear_sigmoid import timed

SHAPES = [(4096, 512, 512)]        # the headline's


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
    torch_fwd = {"softplus": F.softplus, "elu": F.elu}
    torch_gz = {"softplus": lambda g, a: g * (-torch.expm1(-a)), "elu": lambda g, a: torch.ops.aten.elu_backward(g, 1, 1, 1, True, a)}
    gs = [torch.randn(rows, out_f, device=dev) for _ in range(NP)]
    xs = [torch.randn(rows, in_f, device=dev) for _ in range(NP)]
    ws = [torch.randn(out_f, in_f, device=dev) / out_f ** 0.5 for _ in range(NP)]
    bs = [torch.randn(out_f, device=dev) for _ in range(NP)]
    outs = {act: [fn(2.0 * torch.randn(rows, out_f, device=dev)) for _ in range(NP)] for act, fn in torch_fwd.items()}      # a pair's output
    sigs = [torch.sigmoid(torch.randn(rows, out_f, device=dev)) for _ in range(NP)]
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

    sides = [("pn_linear_fwd identity", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0))),
             ("pn_linear_fwd sigmoid", each(lambda i: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0, act="sigmoid"))),
             ("pn_linear_bwd_act sigmoid", each(lambda i: ops.linear_bwd(gs[i], sigs[i], ws[i], gzs[i], dxs[i], flags=0, act="sigmoid"))),
             ("sigmoid_bwd + pn_linear_dx", each(lambda i: ops.linear_dx(sb(gs[i], sigs[i]), ws[i], dxs[i], flags=0)))]
    for act in ("softplus", "elu"):
        a, tf, tg = outs[act], torch_fwd[act], torch_gz[act]
        sides += [
            ("pn_linear_fwd " + act, each(lambda i, act=act: ops.linear_fwd(xs[i], ws[i], bs[i], False, ys[i], flags=0, act=act))),
            ("F.linear + " + act, each(lambda i, tf=tf: tf(F.linear(xs[i], ws[i], bs[i])))),
            ("pn_linear_bwd_act " + act, each(lambda i, act=act, a=a: ops.linear_bwd(gs[i], a[i], ws[i], gzs[i], dxs[i], flags=0, act=act))),
            (act + "_bwd + matmul", each(lambda i, tg=tg, a=a: torch.matmul(tg(gs[i], a[i]), ws[i], out=dxs[i]))),
            (act + "_bwd + pn_linear_dx", each(lambda i, tg=tg, a=a: ops.linear_dx(tg(gs[i], a[i]), ws[i], dxs[i], flags=0))),
        ]
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
    U = 2.0 ** 24
    g, x, w, b = gs[0], xs[0], ws[0], bs[0]
    ident = ops.linear_fwd(x, w, b, False)
    z64 = ident.double()
    for act in ("softplus", "elu"):
        a = outs[act][0]
        y = ops.linear_fwd(x, w, b, False, act=act)
        gz, dx = ops.linear_bwd(g, a, w, act=act)
        gz_t = torch_gz[act](g, a)
        if act == "softplus":
            y64 = torch.clamp(z64, min=0) + torch.log1p(torch.exp(-z64.abs()))
            gz64 = g.double() * (-torch.expm1(-a.double()))
        else:
            y64 = torch.where(z64 > 0, z64, torch.expm1(z64))
            gz64 = torch.where(a.double() > 0, g.double(), g.double() * (a.double() + 1.0))
        rel = torch.clamp(y64.abs(), min=2.0 ** -126)
        print("%s forward: max |y - y64(identity forward)| / |y| = %.2f x 2^-24 (%s on the same z: %.2f);  backward: max |g_z - g_z64| / |g| = "
              "%.2f x 2^-24 (the torch expression: %.2f), dx pn_linear_dx's of g_z bit for bit: %s" % (
                  act, float(((y.double() - y64).abs() / rel).max()) * U, "F." + act,
                  float(((torch_fwd[act](ident).double() - y64).abs() / rel).max()) * U,
                  float(((gz.double() - gz64).abs() / g.double().abs()).max()) * U,
                  float(((gz_t.double() - gz64).abs() / g.double().abs()).max()) * U,
                  torch.equal(dx.view(torch.int32), ops.linear_dx(gz, w).view(torch.int32))))


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
