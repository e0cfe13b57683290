"""The launch sequence of a batch-scope explicit RK solve, forward and backward, is pinned: every ``rk_stage``, ``combine_wrms``,
``adj_*``, ``param_accum*``, ``copy``, ``lincomb``, ``dense_*`` and ``tgrad_*`` / ``dense_tgrad`` call of the sweeps on the CPU
stand-in (tests/_cpu_tgrad_ops.py), as (method name, number of vector terms), against tests/golden/rksweep_trace.json.  The
calls of the C++ step loops come back through the stand-in's ``vec_ops`` table and are seen as well.  The fixture was recorded
by ``record()`` below running on the commit BEFORE the forward sweep moved beside its reverse and both were cut into named
pieces (8283652): a later change of pnode_amd/_rk_sweep.py that adds, drops, reorders or regroups a launch fails here.  It is
never regenerated from the code under test; a change that means to alter the launches says so and records the fixture from its
own parent's behaviour plus the intended difference."""
import json
import os

import pytest
import torch

from _cpu_tgrad_ops import CpuTgradOps
from problems import SpiralTruth
from pnode_amd import options, petsc_adjoint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rksweep_trace.json")
B, D = 3, 2
TIMES = [0.0, 0.03, 0.05, 0.1, 0.12, 0.17, 0.2]
WRAPPED = ("rk_stage", "combine_wrms", "adj_theta", "adj_accum", "param_accum", "param_accum_multi", "copy", "lincomb",
           "dense_eval", "dense_adjoint", "tgrad_dots", "dense_tgrad")
# tableau: (options of the stepper, output modes, first / fixed step): 5f has no continuous extension, -pn_output_times
# interpolate refuses it; the adaptive ones start too long, so that the first attempt is rejected
TABLEAUS = {"5dp": ({"ts_rtol": 1e-6, "ts_atol": 1e-6}, ("match", "interpolate"), 0.05),
            "5f": ({"ts_rtol": 1e-6, "ts_atol": 1e-6}, ("match",), 0.05),
            "4": ({"ts_adapt_type": "none"}, ("match", "interpolate"), 0.02)}
# the last two re-advance from checkpoints (RKSweep._readvance), the last one with stage values behind the checkpoints
TRAJ = {"all": {"ts_trajectory_solution_only": 0}, "sol": {"ts_trajectory_solution_only": 1},
        "cps2": {"ts_trajectory_max_cps_ram": 2, "ts_trajectory_solution_only": 1},
        "cps2st": {"ts_trajectory_max_cps_ram": 2, "ts_trajectory_solution_only": 0}}
CASES = [(rk, mode, traj, loop, False) for rk in TABLEAUS for mode in TABLEAUS[rk][1] for traj in TRAJ for loop in ("native", "python")]
CASES.append(("5dp", "interpolate", "all", "native", True))             # dL/dt


def case_id(case):
    return "-".join(case[:4]) + ("-tgrad" if case[4] else "")


class TracingOps(CpuTgradOps):
    """Every launching call appends (name, number of vector terms): the length of the call's first list argument (the stage
    derivatives, cotangents or queued gradient sets it combines), 0 for a call without one.  Wrapped by instance attribute,
    so the calls the C++ step loops make through ``vec_ops`` (``self.rk_stage(...)`` of the stand-in's table) are seen too."""

    def __init__(self, *args):
        super().__init__(*args)
        self.trace = []
        for name in WRAPPED:
            setattr(self, name, self._traced(name, getattr(self, name)))

    def _traced(self, name, fn):
        def call(*args, **kw):
            terms = next((len(x) for x in args if isinstance(x, (list, tuple))), 0)
            self.trace.append([name + "".join("[%s]" % k for k in sorted(kw)), terms])
            return fn(*args, **kw)
        return call


def record(rk, mode, traj, loop, tgrad):
    options.clear()
    db = dict(TABLEAUS[rk][0], ts_rk_type=rk, pn_output_times=mode, pn_step_loop=loop, **TRAJ[traj])
    for key, val in db.items():
        options.set_option(key, val)
    try:
        r = torch.logspace(-1.3, 0.3, B, dtype=torch.float64)
        y = torch.stack([r, 0.5 * r], dim=1).requires_grad_(True)
        assert tuple(y.shape) == (B, D)
        t = torch.tensor(TIMES, dtype=torch.float64)
        if tgrad:
            t.requires_grad_()
        ode = petsc_adjoint.ODEPetsc(backend=TracingOps)
        ode.setupTS(y, SpiralTruth(), step_size=TABLEAUS[rk][2], method="dopri5", enable_adjoint=True)
        assert ode._native == (loop == "native")
        pred = ode.odeint_adjoint(y, t)
        n_forward = len(ode._ops.trace)
        pred.sum().backward()
        assert (t.grad is not None) == tgrad
        return {"steps": ode.num_steps, "rejections": ode.num_rejections, "forward": ode._ops.trace[:n_forward],
                "backward": ode._ops.trace[n_forward:]}
    finally:
        options.clear()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_sweeps_launch_what_they_launched_before_the_split(case, golden):
    rk, mode, traj, loop, tgrad = case
    want = golden[case_id(case)]
    got = record(*case)
    assert got["steps"] == want["steps"] and got["rejections"] == want["rejections"] and 7 <= want["steps"] <= 48
    names = lambda rec: set(n.split("[")[0] for n, _ in rec["forward"] + rec["backward"])
    relevant = {"rk_stage", "adj_theta", "adj_accum", "copy", "param_accum_multi"}
    if rk != "4":
        relevant.add("combine_wrms")
    if mode == "interpolate":
        relevant |= {"dense_eval", "dense_adjoint"}
    if tgrad:
        relevant |= {"tgrad_dots", "dense_tgrad"}
    assert names(got) == relevant, sorted(names(got) ^ relevant)           # the code under test exercises every path of the mode
    assert names(want) == relevant, sorted(names(want) ^ relevant)         # ... and so did the recording
    for part in ("forward", "backward"):
        assert len(got[part]) == len(want[part]), part
        for k, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, (part, k, g, w)


def test_the_adaptive_cases_reject_and_the_budgeted_ones_readvance(golden):
    """What the cases are there for: a rejected attempt (the forward sweep hands K_0 over to the next attempt) in the adaptive
    ones, and more stage launches in the backward half of the budgeted ones than the states-only trajectory needs."""
    for case in CASES:
        rk, mode, traj, loop, tgrad = case
        g = golden[case_id(case)]
        if rk != "4":
            assert g["rejections"] > 0, case_id(case)
        if traj in ("cps2", "cps2st"):
            sol = golden[case_id((rk, mode, "sol", loop, tgrad))]
            count = lambda rec: sum(1 for n, _ in rec["backward"] if n == "rk_stage")
            assert count(g) > count(sol), case_id(case)


if __name__ == "__main__":          # python tests/test_rksweep_trace.py OUT.json: the recorder (see the module docstring)
    import sys
    with open(sys.argv[1], "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(case_id(c)) + ":" + json.dumps(record(*c), separators=(",", ":")) for c in CASES) + "\n}\n")
