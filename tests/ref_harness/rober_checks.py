"""python rober_checks.py -- the reference's known-answer checks on ROBER (its own test file: an explicit RK, a
Crank-Nicolson and an IMEX solve of the stiff kinetics, each through odeint_adjoint + backward) run the way a
caller of the reference runs them: `petsc4py.init` with the options of that file, `from pnode import petsc_adjoint`,
ODEPetsc().setupTS(...).  The import environment is pnode_amd_ref_plugin.py's (petsc4py -> compat shim, pnode ->
shim package, device entry points -> CPU stand-in).  The truth (SciPy BDF at rtol 1e-11) and the step sizes come from
tests/golden/rober.json.  Prints one JSON line: loss, loss std and the parameter gradients of every solve."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pnode_amd_ref_plugin  # noqa: F401,E402  (petsc4py shim, pnode shim, CPU stand-in for the device entry points)
import numpy as np  # noqa: E402
import petsc4py  # noqa: E402

petsc4py.init(["prog", "-ts_adapt_type", "none", "-ts_trajectory_type", "memory", "-ts_monitor"])
import torch  # noqa: E402
from petsc4py import PETSc  # noqa: E402
from pnode import petsc_adjoint  # noqa: E402
from problems import RoberEX, RoberIM  # noqa: E402
from test_oracle_pins import Rober  # noqa: E402

gold = json.load(open(os.path.join(os.path.dirname(HERE), "golden", "rober.json")))
t = torch.tensor(gold["t"], dtype=torch.float64)
true_y = torch.tensor(gold["true_y"], dtype=torch.float64)
y0 = true_y[0]
step_size = [float(h) for h in (t[1:] - t[:-1]).tolist()]


def run(method, funcs, **setup):
    ode = petsc_adjoint.ODEPetsc()
    ode.setupTS(y0, funcs[0], step_size=step_size, method=method, enable_adjoint=True, **setup)
    pred = ode.odeint_adjoint(y0, t)
    loss = torch.mean(torch.abs(pred - true_y))
    loss.backward()
    std = torch.std(torch.abs(pred - true_y))
    grads = [float(x) for f in funcs for p in f.parameters() for x in p.grad.reshape(-1)]
    return {"loss": loss.item(), "std": std.item(), "grads": grads}


res = {"scalar_type_is_f64": PETSc.ScalarType == np.float64}
res["cn"] = run("cn", [Rober()], implicit_form=True)
fI, fE = RoberIM(), RoberEX()
res["imex"] = run("imex", [fI, fE], implicit_form=True, imex_form=True, func2=fE)
res["rk3"] = run("rk3", [Rober()])
print(json.dumps(res))
