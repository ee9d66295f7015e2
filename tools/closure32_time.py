#!/usr/bin/env python3
"""Float32 against fp64 Smagorinsky closure on an all-periodic uniform n³ box (default 256), medians of `reps` alternated runs:
  kernel  the one-kernel closure force, ins_smagorinsky_force_f32 against ins_smagorinsky_force_f64 (cuda events around `calls` launches);
  step    the extended RK44 step with the closure (θ = 0.17), timesteps32_ against timesteps_ through the fp64 extended loop.
One JSON line per run and one per median; the last line asserts nothing slower: float kernel median <= fp64 kernel median + the runs' spread.
    tools/closure32_time.py [n] [reps] [calls] [steps]"""
import json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ins_amd as ins
from ins_amd import f32

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 50
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
θ = 0.17
x = tuple(np.arange(n + 1) / n for _ in range(3))
setup = ins.Setup(x=x, Re=2000.0)
ps64 = ins.psolver_spectral(setup)
u64 = ins.random_field(setup, 0.0, A=1.0, psolver=ps64)
u32 = f32.to_f32(setup, u64)
m64, m32 = ins.smagorinsky_closure(setup), f32.smagorinsky_closure32(setup)
grid = f"{n}x{n}x{n}"


def kernel_ms(m, u):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(calls):
        m(u, θ)
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


out = {"kernel_f32": [], "kernel_f64": [], "step_f32": [], "step_f64": []}
for m, u in ((m32, u32), (m64, u64)):
    m(u, θ)  # warm
for rep in range(reps):
    for name, m, u in (("kernel_f32", m32, u32), ("kernel_f64", m64, u64)):
        ms = kernel_ms(m, u)
        out[name].append(ms)
        print(json.dumps(dict(case=name, grid=grid, rep=rep, calls=calls, ms=round(ms, 4))), flush=True)

# the extended step with the closure
method = ins.RKMethods.RK44()
s32 = ins.Setup(x=x, Re=2000.0)
s32.closure_model = f32.smagorinsky_closure32(s32)
c32 = f32.ERKCache32(method, s32, f32.psolver_spectral32(s32))
v32 = f32.to_f32(s32, u64)
s64 = ins.Setup(x=x, Re=2000.0)
s64.closure_model = ins.smagorinsky_closure(s64)
p64 = ins.psolver_spectral(s64)
st = ins.create_stepper(method, setup=s64, psolver=p64, u=ins.copyfield(u64))
c64 = ins.ode_method_cache(method, s64, p64)
dt = 1e-4


def step32(k):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    f32.timesteps32_(c32, v32, dt, k, θ=θ)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def step64(k):
    global st
    torch.cuda.synchronize(); t0 = time.perf_counter()
    st = ins.timesteps_(method, st, dt, k, θ=θ, cache=c64)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


step32(2); step64(2)  # warm
for rep in range(reps):
    for name, f in (("step_f32", step32), ("step_f64", step64)):
        ms = f(steps)
        out[name].append(ms)
        print(json.dumps(dict(case=name, grid=grid, method="RK44", rep=rep, steps=steps, ms_per_step=round(ms, 4))), flush=True)
assert bool(torch.isfinite(v32).all())
med = {k: statistics.median(v) for k, v in out.items()}
spread = max(max(v) - min(v) for k, v in out.items() if k.startswith("kernel"))
print(json.dumps(dict(case="medians", grid=grid, **{k: round(v, 4) for k, v in med.items()}, kernel_spread=round(spread, 4),
                      kernel_speedup=round(med["kernel_f64"] / med["kernel_f32"], 3), step_speedup=round(med["step_f64"] / med["step_f32"], 3))), flush=True)
assert med["kernel_f32"] <= med["kernel_f64"] + spread, "the float closure-force kernel is slower than the fp64 one beyond the runs' spread"
