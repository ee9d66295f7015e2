#!/usr/bin/env python3
"""Sensitivity of a Rayleigh-Bénard cell (the setting of RayleighBenard2D.py): the gradient of the lower-plate Nusselt number after a short
run with respect to the initial temperature field, ∂Nu/∂temp0, by reverse mode through `ins.ad.timestep` (temperature equation with viscous
heating and buoyancy, all on the HIP pullback kernels), checked against a central difference in one direction.  With `dtype=torch.float32`
the same problem runs on `ins.ad32` (the reference runs its Rayleigh-Bénard examples in Float32, examples/RayleighBenard2D.jl:71).  With
`rollout=True` the same gradient comes from ONE `ad.timesteps` / `ad32.timesteps` call (the native multi-step loop forward, per-chunk
checkpoints, one native reverse step per step backward), so its memory does not grow with `nstep`.
    python examples/RayleighBenardGradient2D.py n=32 nstep=20 dt=5e-3"""
import numpy as np
import torch

import _common  # noqa: F401
import ins_amd as ins


def main(n=32, nstep=20, dt=5e-3, Pr=0.71, Ra=1e6, Ge=1.0, seed=0, verbose=True, dtype=torch.float64, rollout=False,
         checkpoint_every=None):
    f32 = dtype == torch.float32
    temperature = ins.temperature_equation(
        Pr=Pr, Ra=Ra, Ge=Ge, dodissipation=True, gdir=1, nondim_type=1,
        boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()), (ins.DirichletBC(1.0), ins.DirichletBC(0.0))))
    x = (ins.tanh_grid(0.0, 2.0, 2 * n, 1.2), ins.tanh_grid(0.0, 1.0, n, 1.2))
    walls = (ins.DirichletBC(), ins.DirichletBC())
    setup = ins.Setup(x=x, boundary_conditions=(walls, walls), temperature=temperature)  # Re = 1/α1
    tempfunc = lambda x, y: 0.5 + np.maximum(np.sin(20 * np.pi * x) / 100, 0) + 0 * y  # noqa: E731
    if f32:
        psolver = ins.f32.default_psolver32(setup)
        u0 = ins.f32.vectorfield32(setup)  # at rest
        temp0 = ins.f32.temperaturefield32(setup, tempfunc)
    else:
        psolver = ins.default_psolver(setup)
        u0 = ins.velocityfield(setup, lambda a, x, y: 0 * (x + y), psolver=psolver)
        temp0 = ins.temperaturefield(setup, tempfunc)
    ad = ins.ad32 if f32 else ins.ad
    g = setup.grid
    dy1 = float(g.Δu[1][0])
    dx = torch.as_tensor(np.asarray(g.Δ[0], dtype=np.float64), device=setup.device).to(dtype)
    method = ins.RKMethods.RK44()

    def nusselt(temp):  # lower plate, the formula of RayleighBenard2D.py
        return ((-(temp[:, 1] - temp[:, 0]) / dy1) * dx)[1:-1].sum()

    def run(temp, final=None):
        st = ins.create_stepper(method, setup=setup, psolver=psolver, u=u0, temp=temp)
        if rollout:
            st = ad.timesteps(method, st, dt, nstep, checkpoint_every=checkpoint_every)
        else:
            for _ in range(nstep):
                st = ad.timestep(method, st, dt)
        if final is not None:
            final.append(st.temp.detach())
        return nusselt(st.temp)

    T = temp0.clone().requires_grad_(True)
    final = []
    Nu = run(T, final)
    (grad,) = torch.autograd.grad(Nu, T)
    # one direction, central difference
    gen = torch.Generator(device=setup.device).manual_seed(seed)
    v = ins.f32.scalarfield32(setup) if f32 else ins.scalarfield(setup)
    v.copy_(torch.randn(v.shape, generator=gen, dtype=torch.float64, device=setup.device))
    # Float32: the rounding of Nu enters the difference quotient as about 2^-24 |Nu| / e, so the step sits 30 times higher (Nu is close to linear in
    # temp0 over a short run, so the truncation error, which grows as e^2, stays small)
    e = 3e-2 if f32 else 1e-3
    with torch.no_grad():
        fd = float((run(temp0 + e * v) - run(temp0 - e * v)) / (2 * e))
    dJ = float((grad.double() * v.double()).sum())
    if verbose:
        print(f"Nu(bottom) = {float(Nu.detach()):.6f} after {nstep} steps; <∂Nu/∂temp0, v> = {dJ:.9e}, central difference {fd:.9e}")
    # the plates' ghost volumes are overwritten by the boundary data: no sensitivity there
    return dict(Nu=float(Nu.detach()), grad=grad, dJ=dJ, fd=fd, v=v, temp=final[0], ghost=float(grad[:, 0].abs().max() + grad[:, -1].abs().max()))


if __name__ == "__main__":
    r = main(**_common.cli(dict(n=32, nstep=20, dt=5e-3, Pr=0.71, Ra=1e6, Ge=1.0)))
    print(f"relative difference {abs(r['fd'] - r['dJ']) / abs(r['dJ']):.2e}; max |∂Nu/∂temp0| = {float(r['grad'].abs().max()):.3e}")
