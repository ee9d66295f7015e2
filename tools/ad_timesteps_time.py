"""Time and memory of a differentiable RK44 rollout on a periodic box: `ad.timesteps` with the fused and with the two-launch reverse
stage, against the unrolled loop of `ad.timestep` calls.  Per path: milliseconds per (forward + backward) step, median of `--reps` event-timed
repetitions after `--warmup`, and the peak of torch.cuda.max_memory_allocated over one repetition in vector fields (the work arrays of the native
handles are device allocations of the library and are listed beside it).  One JSON line per measurement.

    python tools/ad_timesteps_time.py [--n 128 256] [--nsteps 8 16] [--reps 5] [--warmup 2] [--out profiles/ad_timesteps_time.jsonl]
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
    for n in a.n:
        x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
        sp = ins.Setup(x=x, Re=1000.0, device="cuda:0")
        ps = ins.psolver_spectral(sp)
        u0 = ins.random_field(sp, 0.0, psolver=ps, seed=2)
        field = u0.numel() * 8
        free, _ = torch.cuda.mem_get_info()

        def rollout(nsteps):
            uu = u0.detach().requires_grad_(True)
            u = ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), 1e-4, nsteps).u
            (u * u).sum().backward()

        def unrolled(nsteps):
            uu = u0.detach().requires_grad_(True)
            st = ins.create_stepper(method, setup=sp, psolver=ps, u=uu)
            for _ in range(nsteps):
                st = ins.ad.timestep(method, st, 1e-4)
            (st.u * st.u).sum().backward()

        for nsteps in a.nsteps:
            for what, on in (("ad.timesteps two-launch reverse stage", 0), ("ad.timesteps fused reverse stage", 1)):
                with ins._lib.options(INS_ADJ_STAGE_FUSED=on):
                    med, lo, hi, peak = measure(lambda: rollout(nsteps), a.reps, a.warmup)
                emit(what=what, n=n, nsteps=nsteps, ms_per_step=med / nsteps, ms_per_step_min=lo / nsteps, ms_per_step_max=hi / nsteps, reps=a.reps,
                     peak_torch_fields=peak / field, library_work_fields=(s + 1) + (2 * s + 1), field_GB=field / 1e9)
            # the unrolled graph keeps about 10 fields per stage alive: run it only where that fits beside what is allocated already
            need = nsteps * s * 12 * field
            if need > free * 0.8:
                emit(what="unrolled ad.timestep loop", n=n, nsteps=nsteps, skipped=f"needs about {need / 1e9:.0f} GB")
                continue
            med, lo, hi, peak = measure(lambda: unrolled(nsteps), a.reps, a.warmup)
            emit(what="unrolled ad.timestep loop", n=n, nsteps=nsteps, ms_per_step=med / nsteps, ms_per_step_min=lo / nsteps, ms_per_step_max=hi / nsteps,
                 reps=a.reps, peak_torch_fields=peak / field, field_GB=field / 1e9)
        del sp, ps, u0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
