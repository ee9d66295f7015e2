"""Time and memory of a differentiable RK44 rollout on a periodic box: `ad.timesteps` with the fused and with the two-launch reverse
stage, against the unrolled loop of `ad.timestep` calls.  Per path: milliseconds per (forward + backward) step, median of `--reps` event-timed
repetitions after `--warmup`, and the peak of torch.cuda.max_memory_allocated over one repetition in vector fields (the work arrays of the native
handles are device allocations of the library and are listed beside it).  One JSON line per measurement.  `--dtype float32` times `ad32.timesteps`
against the unrolled `ad32.timestep` loop, `--temperature` adds the temperature equation (periodic sides, viscous heating on, gravity along z) and
differentiates in (u0, temp0); these run the generic reverse step, which has the two-launch form only.

    python tools/ad_timesteps_time.py [--n 128 256] [--nsteps 8 16] [--reps 5] [--warmup 2] [--dtype float64|float32] [--temperature]
                                      [--out profiles/ad_timesteps_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ins_amd as ins  # noqa: E402


def measure(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts), torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--nsteps", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64")
    ap.add_argument("--temperature", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    method = ins.RKMethods.RK44()
    s = len(method.b)
    f32 = a.dtype == "float32"
    generic = f32 or a.temperature  # the generic reverse step (csrc/ins_rk_adjoint_loop.h)
    ad, name = (ins.ad32, "ad32") if f32 else (ins.ad, "ad")
    tag = dict(dtype=a.dtype, temperature=True) if a.temperature else dict(dtype=a.dtype) if f32 else {}
    for n in a.n:
        x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
        T = None
        if a.temperature:
            per = (ins.PeriodicBC(), ins.PeriodicBC())
            T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, dodissipation=True, gdir=2, boundary_conditions=(per, per, per))
        sp = ins.Setup(x=x, Re=1000.0, device="cuda:0", temperature=T)
        ps = ins.psolver_spectral(sp)
        u0 = ins.random_field(sp, 0.0, psolver=ps, seed=2)
        t0 = ins.temperaturefield(sp, lambda x, y, z: 0.5 + 0.1 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0 * z) if a.temperature else None
        if f32:  # fields built in fp64 and rounded once
            u0 = ins.f32.to_f32(sp, u0)
            t0 = ins.f32.to_f32(sp, t0) if t0 is not None else None
            del ps
            ps = ins.f32.psolver_spectral32(sp)
        field = u0.numel() * u0.element_size()
        free, _ = torch.cuda.mem_get_info()

        def leaves():
            return u0.detach().requires_grad_(True), None if t0 is None else t0.detach().requires_grad_(True)

        def loss(st):
            out = (st.u * st.u).sum()
            return out if st.temp is None else out + (st.temp * st.temp).sum()

        def rollout(nsteps):
            uu, tt = leaves()
            loss(ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu, temp=tt), 1e-4, nsteps)).backward()

        def unrolled(nsteps):
            uu, tt = leaves()
            st = ins.create_stepper(method, setup=sp, psolver=ps, u=uu, temp=tt)
            for _ in range(nsteps):
                st = ad.timestep(method, st, 1e-4)
            loss(st).backward()

        # work arrays of the library in vector fields of this precision: forward cache + reverse step (+ the scalars of the coupled loops)
        work = (s + 1) + (2 * s + 1) + (((2 * s + 1) + (s + 3)) / 3.0 if a.temperature else 0)
        for nsteps in a.nsteps:
            forms = (("two-launch reverse stage", 0),) if generic else (("two-launch reverse stage", 0), ("fused reverse stage", 1))
            for what, on in forms:
                with ins._lib.options(INS_ADJ_STAGE_FUSED=on):
                    med, lo, hi, peak = measure(lambda: rollout(nsteps), a.reps, a.warmup)
                emit(what=f"{name}.timesteps {what}", n=n, nsteps=nsteps, ms_per_step=med / nsteps, ms_per_step_min=lo / nsteps,
                     ms_per_step_max=hi / nsteps, reps=a.reps, peak_torch_fields=peak / field, library_work_fields=work, field_GB=field / 1e9, **tag)
            # the unrolled graph keeps about 10 fields per stage alive: run it only where that fits beside what is allocated already
            need = nsteps * s * 12 * field
            if need > free * 0.8:
                emit(what=f"unrolled {name}.timestep loop", n=n, nsteps=nsteps, skipped=f"needs about {need / 1e9:.0f} GB", **tag)
                continue
            med, lo, hi, peak = measure(lambda: unrolled(nsteps), a.reps, a.warmup)
            emit(what=f"unrolled {name}.timestep loop", n=n, nsteps=nsteps, ms_per_step=med / nsteps, ms_per_step_min=lo / nsteps,
                 ms_per_step_max=hi / nsteps, reps=a.reps, peak_torch_fields=peak / field, field_GB=field / 1e9, **tag)
        del sp, ps, u0, t0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
