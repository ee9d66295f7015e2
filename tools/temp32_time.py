#!/usr/bin/env python3
"""Step time of the Float32 temperature loop on the box of examples/RayleighBenard3D.py (periodic x walls x walls, tanh-stretched, direct solver, RK33C2):
the one-pass stage kernel against the operator-by-operator sequence (INS_DISABLE_TEMP32_STAGE), alternated, and the fp64 step of the same problem through
solve_unsteady.
    tools/temp32_time.py [n] [steps] [reps]          timings, one JSON line each
    tools/temp32_time.py [n] [steps] profile 0|1     only the Float32 steps with INS_DISABLE_TEMP32_STAGE = 0 | 1 (for a kernel trace)"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ins_amd as ins
from ins_amd import _lib, f32

n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
profile = len(sys.argv) > 4 and sys.argv[3] == "profile"
reps = 5 if profile or len(sys.argv) <= 3 else int(sys.argv[3])
dt = 1e-2
temperature = ins.temperature_equation(
    Pr=0.71, Ra=1e7, Ge=1.0, dodissipation=True, gdir=2, nondim_type=1,
    boundary_conditions=((ins.PeriodicBC(), ins.PeriodicBC()), (ins.SymmetricBC(), ins.SymmetricBC()), (ins.DirichletBC(1.0), ins.DirichletBC(0.0))))
x = (np.linspace(0.0, np.pi, 2 * n), ins.tanh_grid(0.0, 1.0, n, 1.2), ins.tanh_grid(0.0, 1.0, n, 1.2))
walls = (ins.DirichletBC(), ins.DirichletBC())
setup = ins.Setup(x=x, boundary_conditions=((ins.PeriodicBC(), ins.PeriodicBC()), walls, walls), temperature=temperature)
ps = ins.psolver_direct(setup)
method = ins.RKMethods.RK33C2()
tempfunc = lambda x, y, z: 0.5 + np.sin(20 * x) * np.sin(20 * np.pi * y) / 100 + 0 * z  # noqa: E731
u64 = ins.velocityfield(setup, lambda a, x, y, z: 0 * (x + y + z), psolver=ps)
t64 = ins.temperaturefield(setup, tempfunc)
ps32 = f32.psolver_wrap32(setup, ps)
cache = f32.ERKCache32(method, setup, ps32)
u, temp = f32.to_f32(setup, u64), f32.temperaturefield32(setup, tempfunc)
shape = "x".join(str(k - 2) for k in setup.grid.N)


def run32(disable, k):
    with _lib.options(INS_DISABLE_TEMP32_STAGE=disable):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f32.timesteps32_(cache, u, dt, k, temp=temp)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


if profile:
    run32(int(sys.argv[4]), steps)
    sys.exit(0)
for d in (0, 1):
    run32(d, 5)  # warm both routes
for rep in range(reps):
    for d in (0, 1):
        ms = run32(d, steps) * 1e3
        print(json.dumps(dict(case="rb3d_f32_step", grid=shape, method="RK33C2", INS_DISABLE_TEMP32_STAGE=d, rep=rep, steps=steps, ms_per_step=round(ms, 4))), flush=True)
assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(temp).all())
state = (u64, t64)
for rep in range(reps + 1):  # first: warm-up
    torch.cuda.synchronize(); t0 = time.perf_counter()
    (u64, t64, _), _ = ins.solve_unsteady(setup=setup, tlims=(0.0, steps * dt), ustart=u64, tempstart=t64, method=method, Δt=dt, psolver=ps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    if rep:
        print(json.dumps(dict(case="rb3d_f64_step_solve_unsteady", grid=shape, method="RK33C2", rep=rep - 1, steps=steps, ms_per_step=round(ms, 4))), flush=True)
