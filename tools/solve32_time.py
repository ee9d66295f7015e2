#!/usr/bin/env python3
"""Timings of the Float32 driver on all-periodic uniform boxes, medians of `reps` alternated runs (host clock around blocking calls):
  cfl    ins_cfl_timestep_f32 (one pass, cached partials) against ins_cfl_timestep_f64 (a cell-sized buffer and a reduction per direction), per box;
  solve  one adaptive Float32 solve_unsteady (cfl = 0.9, n_adapt_Δt = 1) against the same number of steps at fixed Δt, both with a processor that
         looks at every step (no batching), so the share of the CFL evaluation in a step is on record.
One JSON line per median; the last line of each box says whether the float entry is faster.
    tools/solve32_time.py [steps] [reps] [calls] [box ...]        (default 100 3 20 256 512; the solve runs on the first box)"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ins_amd as ins  # noqa: E402
from ins_amd import f32  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
boxes = [int(a) for a in sys.argv[4:]] or [256, 512]


def clock(f, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def cfl_times(n):
    setup = ins.Setup(x=tuple(np.arange(n + 1) / n for _ in range(3)), Re=2000.0)
    u64 = ins.random_field(setup, 0.0, A=1.0, kp=10, psolver=ins.psolver_spectral(setup))
    u32 = f32.to_f32(setup, u64)
    f = {"cfl_f32": lambda: f32.get_cfl_timestep32_(u32, setup), "cfl_f64": lambda: ins.get_cfl_timestep_(None, u64, setup)}
    a, b = f["cfl_f32"](), f["cfl_f64"]()  # warm; the two agree to float rounding
    assert abs(a - b) <= 2.5e-7 * b, (a, b)
    out = {k: [] for k in f}
    for _ in range(reps):
        for k in f:
            out[k].append(clock(f[k], calls))
    med = {k: statistics.median(v) for k, v in out.items()}
    cells = (n + 2) ** 3
    for k, v in med.items():
        print(json.dumps(dict(what=k, grid=f"{n}^3", ms=round(v, 4), runs=[round(x, 4) for x in out[k]], calls=calls,
                              GBps_of_u=round(3 * cells * (4 if k == "cfl_f32" else 8) / v / 1e6, 1))), flush=True)
    print(json.dumps(dict(what="cfl_f32_faster", grid=f"{n}^3", ratio=round(med["cfl_f64"] / med["cfl_f32"], 2), ok=med["cfl_f32"] < med["cfl_f64"])), flush=True)
    return setup, u32


def solve_times(setup, u32, n):
    count = [0]

    def counter():
        return ins.processor(lambda state: state.on(lambda s: count.__setitem__(0, s["n"])))

    ps = f32.psolver_spectral32(setup)
    method = ins.RKMethods.RK44()
    cache = f32.ERKCache32(method, setup, ps)
    cflnum = 0.9
    tend = steps * cflnum * f32.get_cfl_timestep32_(u32, setup)
    kw = dict(setup=setup, ustart=u32, method=method, psolver=ps, cache=cache, tlims=(0.0, tend))

    def adaptive():
        ins.solve_unsteady(cfl=cflnum, n_adapt_Δt=1, processors=dict(c=counter()), **kw)
        return count[0]

    nsteps = adaptive()  # warm, and the number of steps the adaptive run takes

    def fixed():
        ins.solve_unsteady(Δt=tend / nsteps, processors=dict(c=counter()), **kw)
        return count[0]

    assert fixed() == nsteps
    out = {"solve_adaptive": [], "solve_fixed": []}
    for _ in range(reps):
        for k, f in (("solve_adaptive", adaptive), ("solve_fixed", fixed)):
            out[k].append(clock(f, 1) / nsteps)
    med = {k: statistics.median(v) for k, v in out.items()}
    for k, v in med.items():
        print(json.dumps(dict(what=k, grid=f"{n}^3", steps=nsteps, ms_per_step=round(v, 4), runs=[round(x, 4) for x in out[k]])), flush=True)
    print(json.dumps(dict(what="cfl_share_of_adaptive_step", grid=f"{n}^3", share=round(1 - med["solve_fixed"] / med["solve_adaptive"], 4))), flush=True)


first = None
for n in boxes:
    got = cfl_times(n)
    if first is None:
        first = (*got, n)
    else:
        del got
    torch.cuda.empty_cache()
solve_times(*first)
