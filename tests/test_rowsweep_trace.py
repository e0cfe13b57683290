"""The launch sequence of a -pn_adapt_scope sample solve, forward and backward, is pinned: every ``rows_*``, ``copy`` and
``param_accum*`` call of the sweep on the CPU stand-in (tests/_cpu_rows_dense_ops.py), as (method name, number of vector
terms), against tests/golden/rowsweep_trace.json.  The fixture was recorded by ``record()`` below running on the commit
BEFORE the sweep was split into set-up / round / closing pieces (8a8bc7a): a later change of pnode_amd/_rowsweep.py that
adds, drops, reorders or regroups a launch fails here.  It is never regenerated from the code under test; a change that
means to alter the launches says so and records the fixture from its own parent's behaviour plus the intended difference."""
import json
import os

import pytest
import torch

from _cpu_rows_dense_ops import CpuRowsDenseOps
from problems import SpiralTruth
from pnode_amd import options, petsc_adjoint

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowsweep_trace.json")
B, D = 3, 2
TIMES = [0.0, 0.03, 0.05, 0.1, 0.12, 0.17, 0.2]
TOL = {"3bs": 1e-6, "5dp": 1e-8}
CASES = [(rk, mode) for rk in ("3bs", "5dp") for mode in ("match", "interpolate")]


class TracingOps(CpuRowsDenseOps):
    """Every rows_* / copy / param_accum* call appends (name, number of vector terms): the length of the call's first list
    argument (the stage derivatives, cotangents or queued gradient sets it combines), 0 for a call without one.  A
    keyword argument (rows_adj_theta's dense_w) is part of the name."""

    def __init__(self, *args):
        super().__init__(*args)
        self.trace = []
        for name in dir(self):
            if name.startswith("rows_") or name == "copy" or name.startswith("param_accum"):
                setattr(self, name, self._traced(name, getattr(self, name)))

    def _traced(self, name, fn):
        def call(*args, **kw):
            terms = next((len(x) for x in args if isinstance(x, (list, tuple))), 0)
            self.trace.append([name + "".join("[%s]" % k for k in sorted(kw)), terms])
            return fn(*args, **kw)
        return call


def record(rk, mode):
    options.clear()
    options.set_option("ts_rk_type", rk)
    options.set_option("ts_rtol", TOL[rk])
    options.set_option("ts_atol", TOL[rk])
    options.set_option("pn_adapt_scope", "sample")
    options.set_option("pn_output_times", mode)
    try:
        r = torch.logspace(-1.3, 0.3, B, dtype=torch.float64)
        y = torch.stack([r, 0.5 * r], dim=1).requires_grad_(True)
        assert tuple(y.shape) == (B, D)
        ode = petsc_adjoint.ODEPetsc(backend=TracingOps)
        ode.setupTS(y, SpiralTruth(), step_size=0.01, method="dopri5", enable_adjoint=True)
        pred = ode.odeint_adjoint(y, torch.tensor(TIMES, dtype=torch.float64))
        n_forward = len(ode._ops.trace)
        pred.sum().backward()
        return {"rounds": ode.rounds, "forward": ode._ops.trace[:n_forward], "backward": ode._ops.trace[n_forward:]}
    finally:
        options.clear()


@pytest.mark.parametrize("rk,mode", CASES)
def test_the_sweeps_launch_what_they_launched_before_the_split(rk, mode):
    with open(GOLDEN) as fh:
        want = json.load(fh)["%s-%s" % (rk, mode)]
    got = record(rk, mode)
    assert got["rounds"] == want["rounds"] and want["rounds"] > 3
    names = set(n.split("[")[0] for n, _ in want["forward"] + want["backward"])
    assert {"rows_stage", "rows_combine_wrms", "rows_control", "rows_commit", "rows_adj_theta", "rows_adj_accum", "copy",
            "param_accum_multi"} <= names
    assert ("rows_dense_eval" in names) == ("rows_dense_adjoint" in names) == (mode == "interpolate")
    for part in ("forward", "backward"):
        assert len(got[part]) == len(want[part]), part
        for k, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, (part, k, g, w)


if __name__ == "__main__":          # python tests/test_rowsweep_trace.py OUT.json: the recorder (see the module docstring)
    import sys
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(("%s-%s" % c, record(*c)) for c in CASES), fh, separators=(",", ":"))
        fh.write("\n")
