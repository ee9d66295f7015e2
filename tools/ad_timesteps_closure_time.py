"""Time and memory of a differentiable LES rollout with the Smagorinsky closure on a periodic box: `ad.timesteps(…, θ=)` /
`ad32.timesteps(…, θ=)`, the closure inside both native loops, against the route users had before, the unrolled loop of `ad.timestep` calls with
`ad.smagorinsky_closure` as the setup's model.  Both differentiate a quadratic loss in u0 and θ.  Per route: milliseconds per (forward + backward)
step, median, minimum and maximum of `--reps` event-timed repetitions after `--warmup`, and the peak of torch.cuda.max_memory_allocated over the
repetitions in vector fields (the native handles' work arrays are device allocations of the library and are listed beside it).  Also the event time
of the closure pullback alone (ins_smagorinsky_force_pullback_*, with θbar) beside the forward force (ins_smagorinsky_force_*).  One JSON line per
measurement.

    python tools/ad_timesteps_closure_time.py [--n 128] [--nsteps 8] [--reps 5] [--warmup 2] [--dtype float64 float32] [--out FILE.jsonl]
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

THETA, DT = 0.17, 1e-4


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
    ap.add_argument("--n", type=int, nargs="+", default=[128])
    ap.add_argument("--nsteps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", choices=["float64", "float32"], nargs="+", default=["float64", "float32"])
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
        for dname in a.dtype:
            f32 = dname == "float32"
            ad, name, dtype = (ins.ad32, "ad32", torch.float32) if f32 else (ins.ad, "ad", torch.float64)
            x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
            sp = ins.Setup(x=x, Re=1000.0, device="cuda:0")
            ps = ins.psolver_spectral(sp)
            u0 = ins.random_field(sp, 0.0, psolver=ps, seed=2)
            if f32:  # fields built in fp64 and rounded once
                u0 = ins.f32.to_f32(sp, u0)
                del ps
                ps = ins.f32.psolver_spectral32(sp)
            sp.closure_model = ad.smagorinsky_closure(sp)
            field = u0.numel() * u0.element_size()
            tag = dict(n=n, nsteps=a.nsteps, dtype=dname, reps=a.reps, warmup=a.warmup, field_GB=field / 1e9)

            def leaves():
                return u0.detach().requires_grad_(True), torch.tensor(THETA, dtype=dtype, device=sp.device, requires_grad=True)

            def rollout():
                uu, th = leaves()
                (ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), DT, a.nsteps, θ=th).u ** 2).sum().backward()

            def unrolled():
                uu, th = leaves()
                st = ins.create_stepper(method, setup=sp, psolver=ps, u=uu)
                for _ in range(a.nsteps):
                    st = ad.timestep(method, st, DT, th)
                (st.u ** 2).sum().backward()

            # the library's work arrays in vector fields of this precision: forward cache, reverse step, closure force, ∇ubar (D·D scalars; allocated as doubles)
            work = (s + 1) + (2 * s + 1) + 1 + 3 * (2 if f32 else 1)
            for what, fn, extra in ((f"{name}.timesteps with θ (closure in the native loops)", rollout, dict(library_work_fields=work)),
                                    (f"unrolled {name}.timestep loop with {name}.smagorinsky_closure", unrolled, {})):
                med, lo, hi, peak = measure(fn, a.reps, a.warmup)
                emit(what=what, ms_per_step=med / a.nsteps, ms_per_step_min=lo / a.nsteps, ms_per_step_max=hi / a.nsteps, peak_torch_fields=peak / field,
                     **extra, **tag)
                torch.cuda.empty_cache()

            # the operator alone: forward force and its pullback (ubar overwritten, θbar added to)
            u = ins.f32.apply_bc_u32_(u0.clone(), sp) if f32 else ins.apply_bc_u(u0, 0.0, sp)
            sbar = u.clone()
            vec = ins.f32.vectorfield32 if f32 else ins.vectorfield
            sout, ubar, tb = vec(sp), vec(sp), torch.zeros((), dtype=torch.float64, device=sp.device)
            if f32:
                fwd = lambda: ins.f32.smagorinsky_force32_(sout, u, THETA, sp)  # noqa: E731
                bwd = lambda: ins.f32.smagorinsky_force_pullback32_(ubar, tb, sbar, u, THETA, sp)  # noqa: E731
            else:
                fwd = lambda: ins.operators.smagorinsky_force_(sout, u, THETA, sp)  # noqa: E731
                bwd = lambda: ins.operators.smagorinsky_force_pullback_(ubar, tb, sbar, u, THETA, sp)  # noqa: E731
            for what, fn in (("smagorinsky force, forward (one kernel)", fwd), ("smagorinsky force pullback (pass 1, pass 2, tail)", bwd)):
                med, lo, hi, _ = measure(fn, 4 * a.reps, a.warmup)
                emit(what=what, ms=med, ms_min=lo, ms_max=hi, n=n, dtype=dname, reps=4 * a.reps, warmup=a.warmup)
            sp.closure_model = None
            del sp, ps, u0, u, sbar, sout, ubar
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
