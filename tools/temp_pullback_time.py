"""Times of the temperature pullbacks on periodic boxes (DESIGN.md "Differentiability", "Temperature equation"): the fused per-stage entry
(temperature_pullback_) against the four operator-level entries in sequence, momentum_pullback_ on the same box, a flat read + write copy of
the box, and one RK44 step with the temperature equation through ad.timestep (forward only, forward + backward) next to the native step.
One JSON line per measurement; median of `--reps` event-timed repetitions after `--warmup`, all in one process.

    python tools/temp_pullback_time.py [--n 128 256] [--reps 20] [--warmup 3] [--out profiles/r07a_temp_pullback_time.jsonl]
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

BYTES_PER_CELL = 104  # 3-D fused entry, counted from the stencils: u 24 + temp 8 + cbar 8 + Fbar[gdir] 8 read, ubar 48 read + write, tempbar 8 written


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = open(a.out, "w") if a.out else None

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    per = (ins.PeriodicBC(), ins.PeriodicBC())
    method = ins.RKMethods.RK44()
    for n in a.n:
        x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
        for diss in (True, False):
            T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=(per, per, per), dodissipation=diss, gdir=2)
            sp = ins.Setup(x=x, Re=1000.0, temperature=T, device="cuda:0")
            cells = float(np.prod(sp.grid.N))
            u = ins.random_field(sp, 0.0, seed=1)
            Fbar = ins.copyfield(u)
            temp = ins.scalarfield(sp)
            temp.copy_(torch.randn(temp.shape, dtype=torch.float64, device=sp.device, generator=torch.Generator(device=sp.device).manual_seed(2)))
            cbar = ins.copyfield(temp)
            ubar, tempbar = ins.vectorfield(sp), ins.scalarfield(sp)
            tag = dict(n=n, dodissipation=diss)

            ms = timed(lambda: ins.temperature_pullback_(ubar, tempbar, Fbar, cbar, u, temp, sp), a.reps, a.warmup)
            emit(what="temperature_pullback_fused", ms=ms, algorithmic_TBps=BYTES_PER_CELL * cells / ms / 1e9, **tag)

            def sequence():
                tempbar.zero_()
                ins.gravity_adjoint_(tempbar, Fbar, sp)
                ins.convection_diffusion_temp_adjoint_(ubar, tempbar, cbar, u, temp, sp)
                if diss:
                    ins.dissipation_adjoint_(ubar, cbar, u, sp)

            ms = timed(sequence, a.reps, a.warmup)
            emit(what="operator_level_sequence", ms=ms, **tag)
            if diss:
                ms = timed(lambda: ins.momentum_pullback_(ubar, Fbar, u, sp), a.reps, a.warmup)
                emit(what="momentum_pullback", ms=ms, algorithmic_TBps=72 * cells / ms / 1e9, **tag)
                ms = timed(lambda: ubar.copy_(u), a.reps, a.warmup)
                emit(what="copy_vector_field", ms=ms, TBps=48 * cells / ms / 1e9, **tag)
                flat = torch.empty(int(BYTES_PER_CELL * cells / 16), dtype=torch.float64, device=sp.device)
                flat2 = torch.empty_like(flat)
                ms = timed(lambda: flat2.copy_(flat), a.reps, a.warmup)
                emit(what="flat_copy_104B_per_cell", ms=ms, TBps=BYTES_PER_CELL * cells / ms / 1e9, **tag)
                del flat, flat2
            del ubar, tempbar, Fbar, cbar

            # one RK44 step with the temperature equation
            ps = ins.psolver_spectral(sp)
            u0 = ins.random_field(sp, 0.0, psolver=ps, seed=3)
            t0 = ins.apply_bc_temp(0.5 + 0.1 * temp, 0.0, sp)
            cache = ins.ode_method_cache(method, sp, ps)
            un, tn = ins.copyfield(u0), ins.copyfield(t0)

            def native():
                ins.timestep_(method, ins.create_stepper(method, setup=sp, psolver=ps, u=un, temp=tn), 1e-4, cache=cache)

            emit(what="rk44_step_native_forward", ms=timed(native, a.reps, a.warmup), **tag)

            def ad_fwd():
                with torch.no_grad():
                    ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0, temp=t0), 1e-4)

            emit(what="rk44_step_ad_forward_only", ms=timed(ad_fwd, max(3, a.reps // 4), 1), **tag)

            def ad_step():
                uu, tt = u0.detach().requires_grad_(True), t0.detach().requires_grad_(True)
                st = ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu, temp=tt), 1e-4)
                ((st.u * st.u).sum() + (st.temp * st.temp).sum()).backward()

            emit(what="rk44_step_ad_forward_backward", ms=timed(ad_step, max(3, a.reps // 4), 1), **tag)
            del ps, cache, u0, t0, un, tn, u, temp, sp
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
