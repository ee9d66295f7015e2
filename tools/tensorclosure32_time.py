"""Times of the Float32 tensor-basis closure (csrc/ins_tensorclosure32.hip) beside its fp64 twin (csrc/ins_tensorclosure.hip) on a periodic
box, both from the same process and box: tensorinvariants, tensorclosure_stress, the full pullback (stress + invariants
cotangents, abar and ubar), divoftensor and its adjoint, and one RK44 step forward + backward through ad32.timestep with the float32
`neuralclosure.tensorclosure` against ad.timestep with the fp64 one (the same weights).
One JSON line per measurement; median of `--reps` event-timed repetitions after `--warmup`.

    python tools/tensorclosure32_time.py [--n 256] [--reps 20] [--warmup 3] [--no-step]
"""
import argparse

from adjoint_time import emit, timed  # noqa: I001  (puts the repository root on sys.path and imports ins_amd)

import numpy as np
import torch

import ins_amd as ins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="the kernels alone")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    F, n = ins.f32, a.n
    x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
    sp = ins.Setup(x=x, Re=1000.0, device="cuda:0")
    ps64, ps32 = ins.psolver_spectral(sp), F.psolver_spectral32(sp)
    nb, nv, ns = F._tb_sizes(sp)
    cells = float(np.prod(sp.grid.N))
    gen = torch.Generator(device="cuda").manual_seed(0)

    def pair(ncomp):
        f32 = F.nfield32(sp, ncomp)
        f32.copy_(torch.randn(tuple(f32.shape), generator=gen, device=f32.device, dtype=torch.float32))
        f64 = torch.zeros(tuple(reversed(f32.shape)), dtype=torch.float64, device=f32.device).permute(*reversed(range(f32.dim())))
        f64.copy_(f32)
        return f32, f64

    u64 = ins.random_field(sp, 0.0, psolver=ps64, seed=2)
    u32 = F.to_f32(sp, u64)
    a32, a64 = pair(nb)
    t32, t64 = pair(ns)
    v32, v64 = pair(nv)
    w32, w64 = pair(3)
    V32, V64 = pair(nv)
    tau32, tau64 = pair(ns)
    ab32, ab64 = pair(nb)
    ub32, ub64 = pair(3)
    s32, s64 = pair(3)

    # algorithmic bytes per cell: fields read + fields written (the pullback also writes and reads the 9-field ∇ubar scratch)
    rows = [
        ("tensorinvariants", 3 + nv, lambda: ins.tensorinvariants_(V64, u64, sp), lambda: F.tensorinvariants32_(V32, u32, sp)),
        ("tensorclosure_stress", 3 + nb + ns, lambda: ins.tensorclosure_stress_(tau64, u64, a64, sp), lambda: F.tensorclosure_stress32_(tau32, u32, a32, sp)),
        ("tensorclosure_pullback", (3 + ns + nb) + (3 + nb + ns + nv + 9) + (9 + 3),
         lambda: ins.tensorclosure_pullback_(ub64, ab64, t64, v64, u64, a64, sp), lambda: F.tensorclosure_pullback32_(ub32, ab32, t32, v32, u32, a32, sp)),
        ("divoftensor", ns + 3, lambda: ins.divoftensor_(s64, t64, sp), lambda: F.divoftensor32_(s32, t32, sp)),
        ("divoftensor_adjoint", 3 + 2 * ns, lambda: ins.divoftensor_adjoint_(tau64, w64, sp), lambda: F.divoftensor_adjoint32_(tau32, w32, sp)),
    ]
    for what, nfields, f64, f32 in rows:
        ms64, ms32 = timed(f64, a.reps, a.warmup), timed(f32, a.reps, a.warmup)
        emit(what=what + "_f64", n=n, ms=ms64, algorithmic_GBps=8 * nfields * cells / ms64 / 1e6)
        emit(what=what + "_f32", n=n, ms=ms32, algorithmic_GBps=4 * nfields * cells / ms32 / 1e6, f32_over_f64=ms32 / ms64)
    if a.no_step:
        return
    del a32, a64, t32, t64, v32, v64, w32, w64, V32, V64, tau32, tau64, ab32, ab64, ub32, ub64, s32, s64
    torch.cuda.empty_cache()

    nc = ins.neuralclosure
    m64 = nc.tensorclosure(setup=sp, hidden=[8], activation=torch.tanh, rng=0)
    m32 = nc.tensorclosure(setup=sp, hidden=[8], activation=torch.tanh, rng=0, dtype=torch.float32)
    with torch.no_grad():
        m64.layers[-1].weight.mul_(1e-8)
        for p64, p32 in zip(m64.parameters(), m32.parameters()):
            p32.copy_(p64)
    method = ins.RKMethods.RK44()

    def step(ad, ps, u0, m):
        sp.closure_model = m
        uu = u0.detach().requires_grad_(True)
        u = ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), 1e-4).u
        (u * u).sum().backward()
        for q in m.parameters():
            q.grad = None

    ms64 = timed(lambda: step(ins.ad, ps64, u64, m64), a.reps, a.warmup)
    emit(what="rk44_step_tensorclosure_ad_forward_backward_f64", n=n, ms=ms64)
    ms32 = timed(lambda: step(ins.ad32, ps32, u32, m32), a.reps, a.warmup)
    emit(what="rk44_step_tensorclosure_ad32_forward_backward_f32", n=n, ms=ms32, f32_over_f64=ms32 / ms64)
    sp.closure_model = None


if __name__ == "__main__":
    main()
