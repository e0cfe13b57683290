"""CPU: the cases of tests/_krylov_cases.py are what they claim to be, before tests/test_gpu_krylov_steps.py uses them
as the yardstick of the device GMRES kernels (pnode_amd/csrc/pn_krylov.hip): the twin of the device state machine
(tests/_cpu_vecops.py) and its perturbed form decide alike, every case takes the second Gram-Schmidt pass where it says
it does, and the twin's residual estimate is the float64 reference's residual history."""
import pytest
import torch

import _krylov_cases as kc

DTYPES = [torch.float64, torch.float32]
SIZES = [5, 257, 1031, 4099]
KEEP126 = (0, 7, 8, 63, 64, 125)


@pytest.mark.parametrize("m", [1, 12, 126])
def test_the_mirror_of_the_state_block_layout(m):
    """read_state restates layout() of pn_krylov.hip; the library gives two numbers away about it."""
    from pnode_amd._lib import load
    lib = load()
    assert lib.pn_krylov_products_offset(m) == 33 * 16 + 20 == kc.HOFF
    for n in (1, 5, 256, 257, 4099, 4096 * 512 + 5):
        assert lib.pn_krylov_state_doubles(n, m) == kc.state_doubles(n, m)
    L = kc.layout(m)
    assert L["part"] == (L["y"] + m + 1) // 2 * 2 and L["hess"] == kc.HOFF + 3 * (m + 2) and L["y"] == L["g"] + m + 1


def _runs():
    for case in ("plain", "open", "near", "mixed"):
        for n in SIZES:
            yield case, n, 12, 12, None
    for n in (160, 1031):
        yield "slow", n, 126, 126, KEEP126
    yield "tie", 5, 4, 1, None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,n,restart,steps,keep", list(_runs()))
def test_twin_and_perturbed_twin_decide_alike_and_every_case_is_what_it_says(case, n, restart, steps, keep, dtype):
    """Both dtypes: the same decisions launch by launch, rest/ww at least RATIO_MARGIN from 0.25 on every first pass
    (exactly 0.25 in the tie case, which the rule `rest > 0.25 ww` sends to the second pass), and per case:
    near and plain refine every column (plain: w = A V_k is mostly d V_k with d in 2..3, rest/ww is about 0.01), open
    refines none while the vector is longer than the cycle, mixed does both, slow does not stop."""
    tw, pt = kc.twins(case, n, dtype, restart, steps, keep)
    assert kc.decisions(tw) == kc.decisions(pt)
    done = tw.trace[-1].st
    ratios = list(tw.kr.ratio.values())
    if case == "tie":
        assert ratios[0] == 0.25 and tw.trace[1].st["phase"] == 3 and done["second_passes"] >= 1
        return
    assert kc.ratio_margin(tw) >= kc.RATIO_MARGIN and kc.ratio_margin(pt) >= kc.RATIO_MARGIN
    if case in ("near", "plain"):
        assert done["second_passes"] == done["total"] > 0
    if case == "open":
        assert done["second_passes"] == 0 if n > restart else all(r > 0.25 for r in ratios[1:3])
    if case == "mixed":
        assert 0 < done["second_passes"] < done["total"]
    if case == "slow":
        assert done["stop"] == 0 and done["total"] == 126 and done["closed"] == 1 and done["apply"] == 1
    elif n < 2 * restart:                    # the short vector: stopped by convergence before the space is exhausted
        ref = kc.reference(case, n, dtype, restart)
        tol = kc.solve_rtol(n, restart, dtype) * ref.beta
        assert done["stop"] == 1 and done["total"] <= n and all(max(r / tol, tol / r) >= 4.0 for r in ref.rho)
    else:
        assert done["stop"] == 0 and done["total"] == steps


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,n,restart,steps,keep", [r for r in _runs() if r[0] != "tie"])
def test_the_twins_residual_estimate_is_the_residual_history_of_the_reference(case, n, restart, steps, keep, dtype):
    """res after column k against rho_{k+1} = min ||b - A x|| over K_{k+1} of the float64 Arnoldi, every column:
    within 16 |twin - perturbed twin|, at least 64 eps(T) ||b||.  After the close, x has that residual and
    V^T V = I, A V_k = V_{k+1} Hbar_k hold with Hbar recovered from the stored rotations.  (Orthogonality: 64 eps per
    vector where every column was refined; a column that was not -- one pass of classical Gram-Schmidt -- divides what is
    left of the earlier loss by rest/ww > 1/4, the price the 0.25 rule accepts, so the bound grows by 1/(rest/ww) there.)"""
    tw, pt = kc.twins(case, n, dtype, restart, steps, keep)
    ref = kc.reference(case, n, dtype, restart)
    eps, bad, loss = kc.eps_of(dtype), [], 1.0
    for a, b in zip(tw.trace, pt.trace):
        if a.what == "step" and a.st["cur"] == a.k and a.st["phase"] == 1:
            loss /= tw.kr.ratio[(a.k, a.k)]
        if a.what == "step" and a.st["kdone"] == a.k + 1 and a.st["cur"] == a.k and a.k + 1 <= ref.cols:
            tol = max(16.0 * abs(a.st["res"] - b.st["res"]), 64.0 * eps * ref.beta)
            if not abs(a.st["res"] - ref.rho[a.k + 1]) <= tol:
                bad.append((a.k, a.st["res"], ref.rho[a.k + 1], tol))
        q = kc.column_quantities(a, ref, ref.A, ref.b)
        if q["orth"] is not None and not q["orth"] <= 64.0 * eps * (a.k + 2) * loss:
            bad.append((a.k, "orthogonality", q["orth"]))
        if q["arnoldi"] is not None and not q["arnoldi"] <= 64.0 * eps * (a.k + 2):
            bad.append((a.k, "Arnoldi residual", q["arnoldi"]))
        if q["true"] is not None:
            rho = ref.rho[min(a.st["kdone"], ref.cols)]
            if not q["true"] <= rho + 64.0 * eps * ref.beta * (a.st["kdone"] + 1) or not q["gap"] <= 64.0 * eps * (a.st["kdone"] + 1):
                bad.append(("close", q["true"], rho, q["gap"]))
    assert not bad, bad[:8]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_optimal_iterate_of_the_reference_has_the_residual_it_reports(dtype):
    ref = kc.reference("open", 257, dtype, 12)
    for k in (0, 1, 7, 12):
        true = float((ref.b - ref.A @ ref.iterate(k)).norm())
        assert abs(true - ref.rho[k]) <= 1e-12 * ref.beta
    assert all(a >= b for a, b in zip(ref.rho, ref.rho[1:]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,k,factor", [("near", 2, 4.0), ("plain", 5, 2.5)])
def test_the_stop_tolerances_lie_between_two_residuals(case, k, factor, dtype):
    """The stop-column tests put the tolerance at the geometric mean of rho_k and rho_{k+1}.  near: every rho_j is at
    least a factor 4 away (a column gains about 1e-3).  plain gains a factor of about 8.5 per column, so NO tolerance
    is a factor 4 from both neighbours; the geometric mean is the best there is, a factor 2.9, and round-off moves res
    by parts in 1e7 at most.  Either way the twin stops at column k + 1, with atol or with rtol deciding."""
    tol, least = kc.stop_tol(case, dtype, k)
    assert least >= factor
    beta = kc.reference(case, 257, dtype, 12).beta
    for rtol, atol in ((1e-30, tol), (tol / beta, 1e-50)):
        for p in (False, True):
            run = kc.twin_run(case, 257, dtype, 12, p, 12, rtol, atol)
            done = run.trace[-1].st
            assert (done["stop"], done["kdone"], done["total"]) == (1, k + 1, k + 1)
