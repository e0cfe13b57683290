"""TEST SCAFFOLDING shared by tests/test_krylov_steps.py (CPU) and tests/test_gpu_krylov_steps.py (-m gpu): the device
GMRES kernels (pnode_amd/csrc/pn_krylov.hip) launch by launch against the Python twin of their state machine
(tests/_cpu_vecops.py krylov_*) and against a float64 Arnoldi written here.

  read_state      the device state block as the fields the twin keeps (mirrors layout() of pn_krylov.hip)
  StepTwin        the twin with the bookkeeping of the close made visible; perturbed=True: what the device may
                  legitimately do differently (another summation order, fused multiply-adds)
  operator        the five dense float64 operators of the tests
  reference       float64 Arnoldi, residual history, optimal iterates
  Run             one scripted solve, the same code for the device and for the twin, a snapshot after every launch
  Ratios          the two tolerance rules, with the largest observed ratio per group
"""
import copy
import functools

import numpy as np
import torch

from _cpu_vecops import CpuVecOps

# ---- the state block.  MIRRORS layout() and the S_* enum of pnode_amd/csrc/pn_krylov.hip (and kTicketDoubles of
# pn_device.h); tests/test_krylov_steps.py pins the two numbers the library gives away about it.
NTICKET = 33 * 16
NHDR = 20
HOFF = NTICKET + NHDR
HDR = ("stop", "kdone", "cur", "phase", "total", "maxit", "apply", "closed", "beta", "bnorm", "tol", "res", "hk1",
       "rtol", "atol", "brk", "nt", "second_passes")
EXACT = ("stop", "kdone", "cur", "phase", "total", "nt", "closed", "apply", "second_passes")


def layout(m, hoff=HOFF):
    L = {"h": hoff}
    L["d"] = L["h"] + (m + 2)
    L["c"] = L["d"] + (m + 2)
    L["hess"] = L["c"] + (m + 2)
    L["cs"] = L["hess"] + (m + 1) * m
    L["sn"] = L["cs"] + m
    L["g"] = L["sn"] + m
    L["y"] = L["g"] + (m + 1)
    L["part"] = (L["y"] + m + 1) // 2 * 2
    return L


def state_doubles(n, m):
    return layout(m)["part"] + (m + 2) * ((n + 255) // 256 + 1) + 2


def read_state(kr):
    """The device state block of a _KrylovBuffers as a dict: the header scalars by name, h, d, c, the rotated
    Hessenberg columns H[k][0..m], cs, sn, g, y (float64 tensors on the host), `raw` (header to the end of y, for
    bit comparisons) and `ticket`.  Waits for the device."""
    m = kr.m
    L = layout(m, kr.hoff)
    S = kr.state[: L["part"]].cpu()
    st = {name: float(S[kr.hoff - NHDR + i]) for i, name in enumerate(HDR)}
    for name in EXACT:
        st[name] = int(st[name])
    cut = lambda a, count: S[L[a]: L[a] + count].clone()
    st.update(h=cut("h", m + 2), d=cut("d", m + 2), c=cut("c", m + 2), H=cut("hess", (m + 1) * m).view(m, m + 1),
              cs=cut("cs", m), sn=cut("sn", m), g=cut("g", m + 1), y=cut("y", m + 1)[:m])
    st["raw"] = S[kr.hoff - NHDR:].clone()
    st["ticket"] = S[: kr.hoff - NHDR].clone()
    return st


class StepTwin(CpuVecOps):
    """CpuVecOps' restatement of the device state machine, unchanged in what it decides and computes, with what the
    closing kernel leaves in the state block (APPLY, NT, y) recorded too, and rest/ww of every first pass kept
    (kr.ratio[k]: the quantity the second-pass rule compares with 0.25).

    perturbed=True: every product summed in reversed element order, every update evaluated one precision up and rounded
    once to the storage dtype -- another block order and fused multiply-adds, which the device is free to use."""

    def __init__(self, dtype, n, perturbed=False):
        super().__init__(torch.device("cpu"), dtype, n)
        self.perturbed = perturbed

    def krylov_new(self, restart):
        kr = super().krylov_new(restart)
        kr.y = [0.0] * restart
        kr.ratio = {}
        kr.second_passes = 0
        return kr

    def _kr_dot(self, a, b):
        if not self.perturbed:
            return super()._kr_dot(a, b)
        return float(torch.dot(a[: self.n].flip(0).double(), b[: self.n].flip(0).double()))

    def _kr_ratio(self, kr, k):
        ww = float(kr.h[k + 1])
        kr.ratio[(kr.S["total"], k)] = (ww - sum(float(kr.h[j]) ** 2 for j in range(k + 1))) / ww if ww > 0.0 else 0.0

    def _kr_finish_column(self, kr, k, hk1, refined):
        if not refined:
            self._kr_ratio(kr, k)
        super()._kr_finish_column(kr, k, hk1, refined)

    def _kr_update(self, kr, out, w, nt, out2=None):
        if kr.S["phase"] == 2 and not kr.S["closed"]:
            self._kr_ratio(kr, kr.S["cur"])
        if not self.perturbed:
            return super()._kr_update(kr, out, w, nt, out2)
        T, n = self.dtype, self.n
        wide = np.longdouble if T == torch.float64 else np.float64
        coef = lambda c: wide(torch.tensor(c, dtype=T).item())
        acc = coef(kr.c[0]) * w[:n].numpy().astype(wide)
        for j in range(nt):
            acc = acc + coef(kr.c[1 + j]) * kr.V[j][:n].numpy().astype(wide)
        acc = torch.from_numpy(acc.astype(np.float64 if T == torch.float64 else np.float32))
        self._put(out, acc)
        if out2 is not None:
            self._put(out2, acc)

    def krylov_close(self, kr, x):
        S = kr.S
        was_closed, kd = S["closed"], S["kdone"]
        super().krylov_close(kr, x)
        if not was_closed and S["closed"] and kd > 0 and S["stop"] not in (4, 5):      # the device: apply
            S["apply"], S["nt"] = 1, kd
            kr.y[:kd] = kr.c[1: 1 + kd]


def twin_state(kr):
    """The twin's state in the form of read_state."""
    m, S = kr.m, kr.S
    st = {name: S.get(name, 0) for name in HDR}
    st["second_passes"] = kr.second_passes
    t = lambda a, count: torch.tensor(list(a)[:count], dtype=torch.float64)
    st.update(h=kr.h.clone(), d=t(kr.d, m + 2), c=t(kr.c, m + 2), H=torch.tensor(kr.H, dtype=torch.float64), cs=t(kr.cs, m),
              sn=t(kr.sn, m), g=t(kr.g, m + 1), y=t(kr.y, m))
    return st


# ---- the operators: explicit dense float64 matrices, and a right-hand side each
MIXED_SEED = 0
# MIXED_SEED: the smallest seed s >= 0 for which, for every n in (5, 257, 1031, 4099), both dtypes, twin and perturbed
# twin, the first cycle of restart 12 takes the second pass on at least one column and not on at least one other, and
# every column of every case run by the tests keeps rest/ww at least RATIO_MARGIN away from 0.25
# (tests/test_krylov_steps.py asserts all of this; the search is `python tests/_krylov_cases.py`).
RATIO_MARGIN = 0.005
SEEDS = {"tie": 0, "plain": 11, "open": 15, "near": 12, "mixed": MIXED_SEED, "slow": 14}


@functools.lru_cache(maxsize=8)
def operator(case, n):
    """(A [n, n], b [n]) in float64."""
    g = torch.Generator().manual_seed(1000 * SEEDS[case] + n)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    if case == "plain":                  # diagonal + rank 3, nonsymmetric, as in tests/test_gpu_krylov.py.  w = A V_k is
        d = 2.0 + torch.rand(n, generator=g, dtype=torch.float64)       # mostly a multiple of V_k (rest/ww about 0.01):
        A = torch.diag(d) + rn(n, 3) @ rn(3, n) / n                     # EVERY column takes the second pass
    elif case == "open":                 # rest/ww about 0.36 on every column: no second pass; contracts by 3/4 a column
        A = torch.eye(n, dtype=torch.float64) + 0.75 * rn(n, n) / n ** 0.5
    elif case == "near":                 # w = A V_k is almost V_k: more than 3/4 of ||w||^2 cancels on every column
        A = torch.eye(n, dtype=torch.float64) + 1e-3 * rn(n, n) / n ** 0.5
    elif case == "mixed":                # "open" on a subspace of s dimensions that holds most of b, "near" elsewhere:
        s_ = min(6, n - 2)               # no second pass until the Krylov space holds the subspace, one on every column after
        Q = torch.linalg.qr(rn(n, s_)).Q
        A = torch.eye(n, dtype=torch.float64) + 1e-3 * rn(n, n) / n ** 0.5 + 2.0 * Q @ (rn(s_, s_) / s_ ** 0.5) @ Q.T
        return A, Q @ rn(s_) + 0.01 * rn(n) / n ** 0.5
    elif case == "tie":                  # exact in both dtypes: V_0 = e_0, w = (3, 1, 1, 1, 0), ww = 12, rest = 3 = ww / 4
        A = 2.0 * torch.eye(n, dtype=torch.float64)        # EXACTLY: `rest > 0.25 ww` is false, the column is refined
        A[:, 0] = torch.tensor([3.0, 1.0, 1.0, 1.0] + [0.0] * (n - 4), dtype=torch.float64)
        b = torch.zeros(n, dtype=torch.float64)
        b[0] = 4.0
        return A, b
    elif case == "slow":                 # no shift: the field of values surrounds zero, GMRES crawls
        A = rn(n, n) / n ** 0.5
    else:
        raise KeyError(case)
    return A, rn(n)


def eps_of(dtype):
    return torch.finfo(dtype).eps


def solve_rtol(n, restart, dtype):
    """The relative tolerance of the scripted solves: out of reach (the scripts run every column they ask for), except
    where the vector is shorter than the cycle -- there the Krylov space is exhausted before the cycle ends, and a solve
    that went on would divide round-off by round-off; it stops at eps^0.55 instead (the exponent: the first of 0.5, 0.55,
    0.6, ... for which no residual of the reference comes within a factor 4 of the tolerance, in any case and either dtype
    at n = 5; tests/test_krylov_steps.py asserts it)."""
    return eps_of(dtype) ** 0.55 if n < 2 * restart else 1e-45


# ---- the float64 reference
class Reference(object):
    """Arnoldi on a dense float64 A from b with two full passes of modified Gram-Schmidt: V [cols + 1, n], Hbar
    [cols + 1, cols], rho[k] = min ||b - A x|| over x in K_k (rho[0] = ||b||), normA = max_k ||A V_k|| (a lower bound of
    ||A||_2: dividing by it asks more, not less).  Stops early where the Krylov space is exhausted."""

    def __init__(self, A, b, cols):
        n = b.numel()
        self.A, self.b = A, b
        self.beta = float(b.norm())
        if self.beta == 0.0:
            cols = 0
        V = torch.zeros(cols + 1, n, dtype=torch.float64)
        H = torch.zeros(cols + 1, cols, dtype=torch.float64)
        V[0] = b / max(self.beta, 1e-300)
        self.normA, k = 0.0, 0
        while k < cols:
            w = A @ V[k]
            nw = float(w.norm())
            self.normA = max(self.normA, nw)
            for _ in range(2):
                for j in range(k + 1):
                    hj = torch.dot(w, V[j])
                    H[j, k] += hj
                    w = w - hj * V[j]
            H[k + 1, k] = w.norm()
            k += 1
            if float(H[k, k - 1]) <= 1e-13 * nw:
                H[k, k - 1] = 0.0
                break
            V[k] = w / H[k, k - 1]
        self.cols, self.V, self.H = k, V, H
        self.rho, self.ys = [self.beta], [None]
        for j in range(1, k + 1):
            e1 = torch.zeros(j + 1, 1, dtype=torch.float64)
            e1[0] = self.beta
            y = torch.linalg.lstsq(H[: j + 1, :j], e1, driver="gelsd").solution
            self.ys.append(y[:, 0])
            self.rho.append(float((e1 - H[: j + 1, :j] @ y).norm()))

    def iterate(self, k):
        """x_k, the minimiser over K_k."""
        return self.V[:k].T @ self.ys[k] if k else torch.zeros_like(self.b)


def unrotate(st, k):
    """Column k of Hbar (entries 0..k+1) from the stored rotated column and the stored rotations."""
    col = st["H"][k][: k + 2].clone()
    for i in range(k, -1, -1):
        c, s = float(st["cs"][i]), float(st["sn"][i])
        a, b = float(col[i]), float(col[i + 1])
        col[i], col[i + 1] = c * a - s * b, s * a + c * b
    return col


# ---- one scripted solve; the same code drives the device (HipVecOps) and the twin
class Snap(object):
    """What one launch left behind, on the host."""

    def __init__(self, what, k, st, kr, x, status, full):
        self.what, self.k, self.st, self.status = what, k, st, status
        self.V = kr.V.detach().cpu().clone() if full else None
        self.vin, self.w, self.x = kr.vin.detach().cpu().clone(), kr.w.detach().cpu().clone(), x.detach().cpu().clone()


class Run(object):
    def __init__(self, ops, A_T, rhs, x, restart, fused=False, reduce=None, flip=False, keep=None):
        self.ops, self.A_T, self.rhs, self.x, self.m = ops, A_T, rhs, x, restart
        self.fused, self.reduce, self.flip, self.keep = fused, reduce, flip, keep
        self.kr = ops.krylov_new(restart)
        self.device = not isinstance(ops, CpuVecOps)
        self.trace = []
        self.after = None                                    # called after every launch (the pad checks)

    def apply_op(self):
        n, kr = self.ops.n, self.kr
        v = kr.vin[:n]
        out = self.A_T.flip(1) @ v.flip(0) if self.flip else self.A_T @ v
        self.ops.copy(kr.w, out.contiguous())

    def snap(self, what, k=-1):
        status = self.ops.krylov_status(self.kr)             # the host looks after every launch
        st = read_state(self.kr) if self.device else twin_state(self.kr)
        full = self.keep is None or what != "step" or k in self.keep
        self.trace.append(Snap(what, k, st, self.kr, self.x, status, full))
        if self.after is not None:
            self.after(self.trace[-1])
        return self.trace[-1]

    def cycle(self, r, steps, rtol, atol, maxit, first, close=True):
        ops, kr = self.ops, self.kr
        if first:
            ops.lincomb(self.x, [self.rhs], [0.0])
        ops.krylov_begin(kr, r, rtol, atol, maxit, first, self.reduce)
        self.snap("begin")
        for k in range(steps):
            self.apply_op()
            ops.krylov_step(kr, -1 if self.fused else k, self.reduce)
            self.snap("step", k)
        if close:
            ops.krylov_close(kr, self.x)
            self.snap("close")
        return self

    def residual(self):
        """r = rhs - A x, as the host computes it at a restart."""
        ops, kr = self.ops, self.kr
        ops.copy(kr.vin, self.x)
        self.apply_op()
        r = torch.empty_like(self.rhs)
        ops.lincomb(r, [self.rhs, kr.w], [1.0, -1.0])
        return r


def twin_run(case, n, dtype, restart, perturbed, steps, rtol, atol=1e-50, maxit=10000, keep=None, reduce=None, b=None):
    A, b0 = operator(case, n)
    b = b0 if b is None else b
    ops = StepTwin(dtype, n, perturbed)
    run = Run(ops, A.to(dtype), b.to(dtype), torch.zeros(n, dtype=dtype), restart, flip=perturbed, keep=keep, reduce=reduce)
    return run.cycle(run.rhs, steps, rtol, atol, maxit, True)


@functools.lru_cache(maxsize=None)
def twins(case, n, dtype, restart, steps, keep=None):
    """(twin, perturbed twin) after the first cycle of the scripted solve; computed once, shared, never changed:
    second_cycle works on copies."""
    rtol = solve_rtol(n, restart, dtype) if case != "slow" else 1e-30
    return tuple(twin_run(case, n, dtype, restart, p, steps, rtol, keep=keep) for p in (False, True))


def second_cycle(run, r, steps):
    """A copy of a finished first cycle, continued from the residual `r` with first=False (no close)."""
    new = copy.copy(run)
    new.kr, new.x, new.trace = copy.deepcopy(run.kr), run.x.clone(), []
    return new.cycle(r.detach().cpu().to(run.rhs.dtype), steps, 0.0, 0.0, 0, False, close=False)


@functools.lru_cache(maxsize=None)
def reference(case, n, dtype, cols):
    """The reference of the first cycle: the operator is the one the solve applies (A rounded to the storage dtype)."""
    A, b = operator(case, n)
    return Reference(A.to(dtype).double(), b.to(dtype).double(), min(cols, n))


def integer_rhs(n):
    """A right-hand side whose <r, r> is exact in any summation order (small integers): the two forms of the first
    kernel of a cycle then give the same bits."""
    g = torch.Generator().manual_seed(n)
    return torch.randint(-3, 4, (n,), generator=g).double() + 4.0 * (torch.arange(n) == 0)


def stop_tol(case, dtype, k, n=257, restart=12):
    """(tolerance at the geometric mean of rho_k and rho_{k+1} of the reference, the least factor between it and any
    rho_j): a solve with that tolerance stops when column k + 1 is done."""
    ref = reference(case, n, dtype, restart)
    tol = (ref.rho[k] * ref.rho[k + 1]) ** 0.5
    return tol, min(max(r / tol, tol / r) for r in ref.rho)


# ---- tolerances (none is a measured number: each comes from the same inputs, on the CPU)
class Ratios(object):
    """twin-spread (device against twin): 16 |twin - perturbed twin|, at least 16 eps(T) scale.
    reference (device against float64): 8 |twin - reference|, at least 64 eps(T) scale.
    Keeps the largest |device - yardstick| / tolerance seen per group and the failures.

    The spread is the largest seen for that quantity at the columns of the cycle so far, not the one of the column alone.
    One column's |twin - perturbed twin| is a single draw: where the quantity is round-off itself (the second-pass
    products of a near-identity operator, of the size of the basis' loss of orthogonality eps/hk1) the draw comes out
    25 times smaller at one column than at its neighbours, and with the column's own spread the device measured 10.2
    times the tolerance there (mixed, n = 1031, float32, c[0..nt] of column 8; 3.6e-5 against spreads of 9e-6 and 1e-5
    at columns 7 and 10), as did other summation orders on the CPU (1.08).  Round-off accumulates along a cycle, so
    what two legitimate evaluations differed by at an earlier column they may differ by at a later one."""

    def __init__(self, dtype):
        self.eps = eps_of(dtype)
        self.worst, self.failed, self.seen = {}, [], {}

    @staticmethod
    def dist(a, b, vector=False):
        d = torch.as_tensor(a, dtype=torch.float64) - torch.as_tensor(b, dtype=torch.float64)
        if d.numel() == 0:
            return 0.0
        return float(d.norm()) if vector else float(d.abs().max())

    def _note(self, group, name, where, err, tol):
        ratio = err / tol if err == err else float("inf")
        if ratio > self.worst.get(group, (0.0,))[0]:
            self.worst[group] = (ratio, name, where)
        if not ratio <= 1.0:
            self.failed.append("%s %s at %s: %.3e against a tolerance of %.3e (ratio %.2f)" % (group, name, where, err, tol, ratio))

    def spread(self, name, where, dev, twin, pert, scale, vector=False):
        key = (where.split(" step")[0].split(" close")[0].split(" begin")[0], name)
        self.seen[key] = max(self.seen.get(key, 0.0), self.dist(twin, pert, vector))
        tol = max(16.0 * self.seen[key], 16.0 * self.eps * scale)
        self._note("twin", name, where, self.dist(dev, twin, vector), tol)

    def ref(self, name, where, dev, twin, ref, scale, one_sided=False):
        tol = max(8.0 * abs(twin - ref), 64.0 * self.eps * scale)
        self._note("reference", name, where, max(dev - ref, 0.0) if one_sided else abs(dev - ref), tol)

    def report(self, label):
        for group, (ratio, name, where) in sorted(self.worst.items()):
            print("RATIO %s %s: %.4f (%s at %s)" % (label, group, ratio, name, where))

    def check(self, label):
        self.report(label)
        assert not self.failed, "\n".join(self.failed[:20])


def column_quantities(snap, ref_run, A64, b64):
    """What a snapshot is compared on against the float64 reference: (res, max|V^T V - I|, Arnoldi residual of the
    column, true residual, |res - true residual| / ||b||); entries that do not apply are None."""
    st, k = snap.st, snap.k
    out = dict(res=st["res"], orth=None, arnoldi=None, true=None, gap=None)
    if snap.what == "step" and st["kdone"] == k + 1 and snap.V is not None:
        n = b64.numel()
        nv = k + 2 if st["stop"] == 0 else k + 1                 # V_{k+1} is not written once the solve has ended
        V = snap.V[:nv, :n].double()
        out["orth"] = float((V @ V.T - torch.eye(nv, dtype=torch.float64)).abs().max())
        if nv == k + 2:
            out["arnoldi"] = float((A64 @ V[k] - V.T @ unrotate(st, k)).norm()) / ref_run.normA
    if snap.what == "close":
        true = float((b64 - A64 @ snap.x[: b64.numel()].double()).norm())
        out["true"], out["gap"] = true, abs(st["res"] - true) / float(b64.norm())
    return out


def compare(R, dev, twin, pert, ref_run, A64, b64, label, cycle_start=True):
    """One device trace against the twin's, the perturbed twin's and the reference; returns the failures of the exact
    part (the toleranced part goes into R)."""
    exact = []
    assert len(dev.trace) == len(twin.trace) == len(pert.trace)
    beta = ref_run.beta
    for sd, st, sp in zip(dev.trace, twin.trace, pert.trace):
        where = "%s %s %d" % (label, sd.what, sd.k)
        D, T, P = sd.st, st.st, sp.st
        for name in EXACT:
            if D[name] != T[name]:
                exact.append("%s: %s is %r, the twin's %r" % (where, name, D[name], T[name]))
        if tuple(sd.status[:3]) != tuple(st.status[:3]):
            exact.append("%s: status %r, the twin's %r" % (where, sd.status, st.status))
        if exact:
            break                                                # (what follows a different decision is not comparable)
        k, n = sd.k, b64.numel()
        ran = sd.what == "step" and T["cur"] == k and T["kdone"] == k + 1      # this launch finished column k
        if sd.what == "begin":
            R.spread("beta", where, D["beta"], T["beta"], P["beta"], beta)
            R.spread("res", where, D["res"], T["res"], P["res"], beta)
            R.ref("beta", where, D["beta"], T["beta"], beta, beta)
            if T["stop"] == 0:
                R.spread("c[0]", where, D["c"][0] * beta, T["c"][0] * beta, P["c"][0] * beta, 1.0)
                R.spread("g[0]", where, D["g"][0], T["g"][0], P["g"][0], beta)
                if sd.V is not None:
                    assert torch.equal(sd.V[0, :n], sd.vin[:n]), where + ": V[0] and vin differ"
                    R.spread("V[0]", where, sd.V[0, :n], st.V[0, :n], sp.V[0, :n], 1.0, vector=True)
        if ran:
            wn = float(unrotate(T, k).norm())                    # ||w|| of the column, to round-off
            R.spread("hess[k]", where, D["H"][k][: k + 2], T["H"][k][: k + 2], P["H"][k][: k + 2], wn)
            for name in ("cs", "sn"):
                R.spread(name + "[k]", where, D[name][k], T[name][k], P[name][k], 1.0)
            R.spread("g[k]", where, D["g"][k], T["g"][k], P["g"][k], beta)
            R.spread("g[k+1]", where, D["g"][k + 1], T["g"][k + 1], P["g"][k + 1], beta)
            R.spread("res", where, D["res"], T["res"], P["res"], beta)
            R.spread("hk1", where, D["hk1"], T["hk1"], P["hk1"], wn)
            nt = T["nt"]
            if T["hk1"] > 0.0:                                   # the table of the update: multiples of 1/hk1
                sc = T["hk1"]
                R.spread("c[0..nt]", where, D["c"][: nt + 1] * sc, T["c"][: nt + 1] * sc, P["c"][: nt + 1] * sc, wn)
            if T["phase"] == 3:
                R.spread("d[0..k]", where, D["d"][: k + 1], T["d"][: k + 1], P["d"][: k + 1], wn)
            if T["stop"] == 0 and sd.V is not None:
                assert torch.equal(sd.V[k + 1, :n], sd.vin[:n]), where + ": V[k+1] and vin differ"
                R.spread("V[k+1]", where, sd.V[k + 1, :n], st.V[k + 1, :n], sp.V[k + 1, :n], 1.0, vector=True)
            if cycle_start and k + 1 <= ref_run.cols:
                R.ref("res", where, D["res"], T["res"], ref_run.rho[k + 1], beta)
        if sd.what == "close" and T["apply"] == 1:
            kd = T["kdone"]
            ysc = max(float(T["y"][:kd].abs().max()), 1e-300)    # y against its own size
            R.spread("y", where, D["y"][:kd] / ysc, T["y"][:kd] / ysc, P["y"][:kd] / ysc, 1.0)
            R.spread("x", where, sd.x[:n], st.x[:n], sp.x[:n], float(st.x[:n].double().norm()), vector=True)
        qd, qt = column_quantities(sd, ref_run, A64, b64), column_quantities(st, ref_run, A64, b64)
        if qd["orth"] is not None:
            R.ref("max|V^T V - I|", where, qd["orth"], qt["orth"], 0.0, 1.0)
        if qd["arnoldi"] is not None:
            R.ref("Arnoldi residual", where, qd["arnoldi"], qt["arnoldi"], 0.0, 1.0)
        if qd["true"] is not None and cycle_start:
            rho = ref_run.rho[min(T["kdone"], ref_run.cols)]
            R.ref("||b - A x|| against the optimum", where, qd["true"], qt["true"], rho, beta, one_sided=True)
            R.ref("|res - ||b - A x||| / ||b||", where, qd["gap"], qt["gap"], 0.0, 1.0)
    return exact


def decisions(run):
    """What a run decided, launch by launch."""
    return [tuple(s.st[name] for name in EXACT) + tuple(s.status[:3]) for s in run.trace]


def ratio_margin(run):
    """The least distance of rest/ww from 0.25 over the first passes of a run."""
    return min([abs(r - 0.25) for r in run.kr.ratio.values()] or [1.0])


def search_mixed_seed(limit=200):                            # pragma: no cover -- run by hand
    global MIXED_SEED
    for seed in range(limit):
        SEEDS["mixed"] = seed
        operator.cache_clear()
        ok = True
        for n in (5, 257, 1031, 4099):
            for dtype in (torch.float64, torch.float32):
                for p in (False, True):
                    run = twin_run("mixed", n, dtype, 12, p, 12, solve_rtol(n, 12, dtype))
                    done = run.trace[-1].st
                    kinds = {r <= 0.25 for r in run.kr.ratio.values()}
                    ok = ok and kinds == {True, False} and ratio_margin(run) >= RATIO_MARGIN and done["second_passes"] < done["total"]
                if not ok:
                    break
            if not ok:
                break
        print("seed", seed, "ok" if ok else "no")
        if ok:
            return seed


if __name__ == "__main__":
    search_mixed_seed()
