"""Times of the reverse-mode layer on periodic boxes (DESIGN.md "Differentiability"): the fused momentum pullback (tiled and generic) against the forward
momentum! pass at 256^3 and 512^3, the project pullback against project!, and one RK44 step through ad.timestep (forward + backward) next to
the native forward step.  The Float32 leg (`f32_leg`, last; `--f32-only` runs it alone) times ins_momentum_pullback_f32, ins_project_pullback_f32
and one RK44 step through ad32.timestep on the `--step-n` box, each beside its fp64 twin from the same process and box.
One JSON line per measurement; median of `--reps` event-timed repetitions after `--warmup`.

    python tools/adjoint_time.py [--n 256 512] [--reps 20] [--warmup 3] [--f32-only]
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def f32_leg(n, reps, warmup):
    F = ins.f32
    x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
    sp = ins.Setup(x=x, Re=1000.0, device="cuda:0")
    ps64, ps32 = ins.psolver_spectral(sp), F.psolver_spectral32(sp)
    method = ins.RKMethods.RK44()
    u64 = ins.random_field(sp, 0.0, psolver=ps64, seed=2)
    u32 = F.to_f32(sp, u64)
    phi64, phi32 = ins.copyfield(u64), ins.copyfield(u32)
    ub64, ub32 = ins.vectorfield(sp), F.vectorfield32(sp)
    pw64, pw32 = ins.scalarfield(sp), F.scalarfield32(sp)
    cells = float(np.prod(sp.grid.N))
    for name, off in (("momentum_pullback_f64_tiled", 0), ("momentum_pullback_f64_generic", 1)):
        with ins._lib.options(INS_DISABLE_ADJ_TILED=off):
            ms = timed(lambda: ins.momentum_pullback_(ub64, phi64, u64, sp), reps, warmup)
        emit(what=name, n=n, ms=ms, algorithmic_GBps=72 * cells / ms / 1e6)
    ms = timed(lambda: F.momentum_pullback32_(ub32, phi32, u32, sp), reps, warmup)
    emit(what="momentum_pullback_f32", n=n, ms=ms, algorithmic_GBps=36 * cells / ms / 1e6)
    emit(what="project_pullback_f64", n=n, ms=timed(lambda: ins.project_pullback_(phi64, sp, ps64, pw64), reps, warmup))
    emit(what="project_pullback_f32", n=n, ms=timed(lambda: F.project_pullback32_(phi32, sp, ps32, pw32), reps, warmup))
    del phi64, phi32, ub64, ub32, pw64, pw32

    def step(ad, ps, u0):
        uu = u0.detach().requires_grad_(True)
        u = ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), 1e-4).u
        (u * u).sum().backward()

    emit(what="rk44_step_ad_forward_backward_f64", n=n, ms=timed(lambda: step(ins.ad, ps64, u64), max(3, reps // 4), 1))
    emit(what="rk44_step_ad32_forward_backward_f32", n=n, ms=timed(lambda: step(ins.ad32, ps32, u32), max(3, reps // 4), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--step-n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pullback-only", action="store_true", help="the momentum pullback kernels alone (counter runs)")
    ap.add_argument("--f32-only", action="store_true", help="the Float32 leg alone")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.f32_only:
        return f32_leg(a.step_n, a.reps, a.warmup)
    for n in a.n:
        x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
        sp = ins.Setup(x=x, Re=1000.0, device="cuda:0")
        u = ins.random_field(sp, 0.0, seed=1)
        phi = ins.copyfield(u)
        ubar, F = ins.vectorfield(sp), ins.vectorfield(sp)
        cells = float(np.prod(sp.grid.N))
        for name, off in (("momentum_pullback_tiled", 0), ("momentum_pullback_generic", 1)):
            with ins._lib.options(INS_DISABLE_ADJ_TILED=off):
                ms = timed(lambda: ins.momentum_pullback_(ubar, phi, u, sp), a.reps, a.warmup)
            emit(what=name, n=n, ms=ms, algorithmic_GBps=72 * cells / ms / 1e6)
        if a.pullback_only:
            del u, phi, ubar, F, sp
            torch.cuda.empty_cache()
            continue
        ms = timed(lambda: ins.momentum_(F, u, None, 0.0, sp), a.reps, a.warmup)
        emit(what="momentum_forward", n=n, ms=ms, algorithmic_GBps=48 * cells / ms / 1e6)
        if n == a.step_n:
            ps = ins.psolver_spectral(sp)
            pw = ins.scalarfield(sp)
            ms = timed(lambda: ins.project_pullback_(phi, sp, ps, pw), a.reps, a.warmup)
            emit(what="project_pullback", n=n, ms=ms)
            ms = timed(lambda: ins.project_(F, sp, ps, pw), a.reps, a.warmup)
            emit(what="project_forward", n=n, ms=ms)
            del ps
        del u, phi, ubar, F, sp
        torch.cuda.empty_cache()
    if a.pullback_only:
        return
    n = a.step_n
    x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
    sp = ins.Setup(x=x, Re=1000.0, device="cuda:0")
    ps = ins.psolver_spectral(sp)
    method = ins.RKMethods.RK44()
    u0 = ins.random_field(sp, 0.0, psolver=ps, seed=2)
    cache = ins.ode_method_cache(method, sp, ps)
    un = ins.copyfield(u0)

    def native():
        ins.timestep_(method, ins.create_stepper(method, setup=sp, psolver=ps, u=un), 1e-4, cache=cache)

    emit(what="rk44_step_native_forward", n=n, ms=timed(native, a.reps, a.warmup))

    def ad_step():
        uu = u0.detach().requires_grad_(True)
        u = ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), 1e-4).u
        (u * u).sum().backward()

    emit(what="rk44_step_ad_forward_backward", n=n, ms=timed(ad_step, max(3, a.reps // 4), 1))

    def ad_fwd():
        with torch.no_grad():
            ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), 1e-4)

    emit(what="rk44_step_ad_forward_only", n=n, ms=timed(ad_fwd, max(3, a.reps // 4), 1))
    del sp, ps, cache, un, u0
    torch.cuda.empty_cache()
    f32_leg(a.step_n, a.reps, a.warmup)


if __name__ == "__main__":
    main()
