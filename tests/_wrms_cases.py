"""TEST SCAFFOLDING -- the plain reference of the weighted RMS error norm and the operand regimes it is tested on
(tests/test_error_norm_host.py on the CPU stand-ins, tests/test_gpu_error_norm.py on the kernels).

A case is a pair (un, err) in the storage type plus (atol, rtol).  Fed as u = un, K_1 = err, ce = [1] (and h = 1), first same as
last, the kernel's err is K_1 bit for bit -- (T)(h * ce) = 1 and fma(1, k, 0) = k are exact -- so the reference needs no model of
the fma chain: uhat = un + err rounded once to the storage type, which numpy does in that type.

Regime classes, interleaved element by element (11 or 7 classes: coprime to the vector width, the wave and the workgroup, so
every lane and vector slot meets every class).  ulp is the spacing of the storage type at |un|, err has the sign of un:
  A1 |err| = ulp / 4 (uhat == u, the term is exactly 0)    A2 err = 1 ulp or 8 ulp (u - uhat exact)
  A3 err = 0.75 ulp (uhat moves a whole ulp)               A4 err = 1.5 ulp (a tie: rounds to even)
  B1 err = +u / 2 (|uhat| > |u|)    B2 err = -u / 2 (|uhat| < |u|)    B3 err = -2.5 u (sign flips, |uhat| = 1.5 |u|)
  C1 un = +0.0, err != 0    C2 un = -0.0, err != 0    C3 err = 0, un != 0    C4 both zero
  E  un ~ 7e19, err = un / 8 with atol = 1e-6, rtol = 0: q ~ 1e25 is finite in fp32 and q * q is not.
Every class is asserted on the constructed arrays, so a typo cannot move a case into another regime unnoticed."""
import math

import numpy as np

CLASSES = ["A1", "B1", "A2", "C1", "A3", "B2", "C3", "A4", "C2", "B3", "C4"]
NO_ZERO = [c for c in CLASSES if c[0] != "C"]          # with atol = 0 a zero pair has tol = 0
PAIRS = [(1e-5, 1e-4), (1e-6, 0.0), (0.0, 1e-3)]
E_PAIR = (1e-6, 0.0)


def wrms_ref(un, uh, atol, rtol):
    """sqrt(mean(((un - uh) / (atol + rtol max(|un|, |uh|)))^2)) of the two STORED solutions: fp64, exactly rounded sum."""
    a, b = np.asarray(un, dtype=np.float64).ravel(), np.asarray(uh, dtype=np.float64).ravel()
    tol = atol + rtol * np.maximum(np.abs(a), np.abs(b))
    q = (a - b) / tol
    return math.sqrt(math.fsum((q * q).tolist()) / a.size)


def stored_uhat(un, err):
    """un + err rounded once to the storage type (numpy adds in that type)."""
    assert un.dtype == err.dtype and un.dtype in (np.float32, np.float64)
    return (un + err).astype(un.dtype)


def _exact(x, T):
    """x (extended precision) is representable in T."""
    return bool(np.all(np.asarray(x, dtype=T).astype(np.longdouble) == np.asarray(x, dtype=np.longdouble)))


def build(T, n, cycle, active=None, e_class=False, dyadic=False):
    """(un, err, class name per element).  `cycle`: the classes in element order; `active`: only elements of this class keep their
    err (the others get err = 0, an exactly zero term, so the class decides the norm alone); `e_class`: a few elements are class
    E; `dyadic`: 4-bit mantissas throughout (the write path needs every product and sum exact)."""
    T = np.dtype(T).type
    i = np.arange(n)
    mag = (1.0 + (i % 8) / 8.0) * 2.0 ** ((i // 8) % 7 - 3)
    sign = np.where((i // 3) % 2 == 1, -1.0, 1.0)
    frac = np.zeros(n) if dyadic else ((i * 7919) % 4093) / 32768.0
    cls = np.array([cycle[k % len(cycle)] for k in range(n)])
    full = np.array([c in ("B1", "B2", "C3") for c in cls])        # full mantissas where the construction stays exact
    odd = (i // len(cycle)) % 2 == 1
    un = (sign * mag * np.where(full, 1.0 + frac, 1.0)).astype(T)
    un = np.where((cls == "A4") & odd, (un + sign.astype(T) * np.spacing(np.abs(un))).astype(T), un).astype(T)   # odd mantissa
    ulp = np.spacing(np.abs(un)).astype(np.float64)
    s = np.sign(un).astype(np.float64)
    err = np.zeros(n)
    pick = {"A1": s * ulp / 4, "A2": s * ulp * np.where(odd, 8.0, 1.0), "A3": s * 0.75 * ulp, "A4": s * 1.5 * ulp,
            "B1": 0.5 * un.astype(np.float64), "B2": -0.5 * un.astype(np.float64), "B3": -2.5 * un.astype(np.float64),
            "C1": sign * mag / 1024.0, "C2": -sign * mag / 1024.0, "C3": np.zeros(n), "C4": np.zeros(n)}
    for c, v in pick.items():
        err = np.where(cls == c, v, err)
    un = np.where(cls == "C1", T(0.0), un).astype(T)
    un = np.where(cls == "C2", T(-0.0), un).astype(T)
    un = np.where(cls == "C4", T(0.0), un).astype(T)
    if e_class:
        at = np.zeros(n, dtype=bool)
        at[[0, n // 2, n - 1]] = True
        at[5::97] = True
        big = (sign * mag * 2.0 ** 66).astype(T)
        un = np.where(at, big, un).astype(T)
        err = np.where(at, big.astype(np.float64) / 8.0, err)
        cls = np.where(at, "E", cls)
    if active is not None:
        err = np.where(cls == active, err, 0.0)
        zero_pair = (cls != active) & (un == 0)
        cls = np.where(cls == active, cls, np.where(zero_pair, "C4", "C3"))
        assert (cls == active).any() or n < len(cycle), active
    assert _exact(err, T)
    err = err.astype(T)
    _check(T, un, err, cls)
    return un, err, cls


def _check(T, un, err, cls):
    """The property that names each class, on the arrays themselves."""
    uh = stored_uhat(un, err)
    u64, e64, h64 = un.astype(np.float64), err.astype(np.float64), uh.astype(np.float64)
    ulp = np.spacing(np.abs(un)).astype(np.float64)
    assert np.isfinite(u64).all() and np.isfinite(e64).all() and np.isfinite(h64).all()
    tiny = np.finfo(T).tiny
    assert ((np.abs(u64) >= tiny) | (u64 == 0)).all() and ((np.abs(e64) >= tiny) | (e64 == 0)).all()       # no denormals
    m = cls == "A1"
    assert (np.abs(e64[m]) == ulp[m] / 4).all() and (uh[m] == un[m]).all() and (T(1) * (un[m] + err[m]) == un[m]).all()
    m = cls == "A2"
    assert np.isin(np.abs(e64[m]) / ulp[m], (1.0, 8.0)).all() and (h64[m] - u64[m] == e64[m]).all()
    m = cls == "A3"
    assert (np.abs(e64[m]) == 0.75 * ulp[m]).all() and (np.abs(h64[m] - u64[m]) == ulp[m]).all()
    m = cls == "A4"
    moved = np.abs(h64[m] - u64[m]) / ulp[m]
    assert (np.abs(e64[m]) == 1.5 * ulp[m]).all() and np.isin(moved, (1.0, 2.0)).all()
    assert ((np.abs(h64[m]) / ulp[m]) % 2 == 0).all()                                                     # the even neighbour
    assert m.sum() < 4 or (set(moved.tolist()) == {1.0, 2.0})                                             # both directions occur
    m = cls == "B1"
    assert (np.sign(h64[m]) == np.sign(u64[m])).all() and (np.abs(h64[m]) > 1.4 * np.abs(u64[m])).all()
    m = cls == "B2"
    assert (np.sign(h64[m]) == np.sign(u64[m])).all() and (np.abs(h64[m]) < 0.6 * np.abs(u64[m])).all() and (h64[m] != 0).all()
    m = cls == "B3"
    assert (np.sign(h64[m]) == -np.sign(u64[m])).all() and (np.abs(h64[m]) == 1.5 * np.abs(u64[m])).all() and (u64[m] != 0).all()
    m = cls == "C1"
    assert (un[m] == 0).all() and (~np.signbit(un[m])).all() and (err[m] != 0).all()
    m = cls == "C2"
    assert (un[m] == 0).all() and np.signbit(un[m]).all() and (err[m] != 0).all()
    m = cls == "C3"
    assert (err[m] == 0).all() and (un[m] != 0).all()
    m = cls == "C4"
    assert (un[m] == 0).all() and (err[m] == 0).all()
    m = cls == "E"
    if m.any():
        atol, rtol = E_PAIR
        with np.errstate(over="ignore"):
            f = np.float32
            tol = f(atol) + f(rtol) * np.maximum(np.abs(un[m].astype(f)), np.abs(uh[m].astype(f)))
            q = (un[m].astype(f) - uh[m].astype(f)) / tol
            assert np.isfinite(q).all() and (np.abs(q) > 1e24).all() and np.isinf(q * q).all()          # fp32 squares overflow
        assert np.isfinite(wrms_ref(un, uh, atol, rtol))


def cases(T, n, dyadic=False):
    """[(name, un, err, atol, rtol)]: per tolerance pair the interleaved mix and every class on its own (the others' terms exactly
    zero: a regime with small terms is not drowned by one with large terms); every element A1; the mix with class E."""
    out = []
    for k, (atol, rtol) in enumerate(PAIRS):
        cycle = CLASSES if atol > 0 else NO_ZERO
        for active in [None] + cycle:
            un, err, cls = build(T, n, cycle, active, dyadic=dyadic)
            if atol == 0:
                uh = stored_uhat(un, err)
                assert (np.maximum(np.abs(un), np.abs(uh)) > 0).all() and rtol > 0                        # no element has tol = 0
            out.append(("pair%d-%s" % (k, active or "mix"), un, err, atol, rtol))
    un, err, cls = build(T, n, ["A1"], dyadic=dyadic)
    assert (cls == "A1").all()
    out.append(("all-A1", un, err) + PAIRS[0])
    un, err, cls = build(T, n, CLASSES, e_class=True, dyadic=dyadic)
    assert (cls == "E").sum() >= 1
    out.append(("E", un, err) + E_PAIR)
    return out


# ---- the write path: unew = u + sum_j cb_j K_j and err = sum_j ce_j K_j with nk = 3, every fma of both chains exact
WRITE_CB = [0.5, 0.25, 8.0]
WRITE_CE = [0.125, 0.0625, 1.0]


def write_path_operands(T, un, err):
    """(u, [K1, K2, K3]) such that the kernel's chains give unew == un and err == err bit for bit: K1 = 4 w and K2 = -8 w cancel in
    both chains (partial sums u + 2 w and w / 2 on the way), K3 = err carries the error, u = un - 8 err.  Every intermediate is
    asserted representable in T, so the fp64 (here: extended) reference cast down is the exact result."""
    T = np.dtype(T).type
    L = np.longdouble
    assert np.finfo(L).nmant >= 63
    n = un.size
    u = un.astype(L) - 8 * err.astype(L)
    assert _exact(u, T)
    u = u.astype(T)
    # w pulls the partial sum u + 2 w towards zero: it never crosses into a binade with a coarser spacing
    scale = np.where(un != 0, np.abs(un.astype(np.float64)), np.abs(err.astype(np.float64)))
    scale = np.where(scale != 0, scale, 1.0)
    w = -np.where(u < 0, -1.0, 1.0) * (1 + np.arange(n) % 5) * 2.0 ** (np.floor(np.log2(scale)) - 6)
    assert _exact(w, T)
    w = w.astype(T)
    K = [(4 * w).astype(T), (-8 * w).astype(T), err.copy()]
    acc_u, acc_e = u.astype(L), np.zeros(n, dtype=L)
    for cb, ce, k in zip(WRITE_CB, WRITE_CE, K):
        acc_u = acc_u + L(cb) * k.astype(L)
        acc_e = acc_e + L(ce) * k.astype(L)
        assert _exact(acc_u, T) and _exact(acc_e, T)
    assert (acc_u.astype(T) == un).all() and (acc_e.astype(T) == err).all()
    return u, K, acc_u.astype(T)
