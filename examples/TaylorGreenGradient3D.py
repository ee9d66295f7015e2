#!/usr/bin/env python3
"""Sensitivity of a Taylor-Green vortex (the setting of TaylorGreenVortex3D.py): the gradient of the final kinetic energy after `nsteps` RK44 steps with
respect to the initial velocity field, by reverse mode through `ins.ad.timesteps` — the native multi-step loop forward, per-chunk checkpoints, and one
native reverse-step call per step backward, so the memory is that of a few fields however long the rollout —, checked against a central difference in
one direction.  With `dtype=torch.float32` the same runs on `ins.ad32.timesteps` and the Float32 spectral solver (the reference recommends single
precision on GPUs); the central difference is then taken at a step 100 times larger, and held to `FD_TOL32`.
    python examples/TaylorGreenGradient3D.py n=32 nsteps=8 dt=1e-3"""
import numpy as np
import torch

import _common  # noqa: F401
import ins_amd as ins

# Float32: the rounding of E enters the difference quotient as about 2^-24 |E| / e; at e = 1e-2 |u0| that is 6e-6 |E|, and <g, v> is of the order of |E|,
# while the e² term (the energy is close to quadratic in u0 over a short run) stays under 1e-4 of it
FD_TOL32 = 1e-3
FD_TOL = 1e-6  # relative: the energy is smooth in u0, so at e = 1e-4 |u0| the central difference is off by its e² term and by eps |E| / e, both under 1e-8


def main(n=32, nsteps=8, dt=1e-3, Re=1600.0, checkpoint_every=None, seed=0, verbose=True, dtype=torch.float64):
    x = tuple(np.linspace(0.0, 2 * np.pi, n + 1) for _ in range(3))
    setup = ins.Setup(x=x, Re=Re)
    f32 = dtype == torch.float32
    ad = ins.ad32 if f32 else ins.ad
    psolver = ins.psolver_spectral(setup)

    def tgv(a, x, y, z):
        if a == 0:
            return np.sin(x) * np.cos(y) * np.cos(z)
        if a == 1:
            return -np.cos(x) * np.sin(y) * np.cos(z)
        return 0 * (x + y + z)

    u0 = ins.velocityfield(setup, tgv, psolver=psolver)
    if f32:  # the start field is built in fp64 and rounded once
        psolver64, psolver = psolver, ins.f32.psolver_spectral32(setup)
        u0 = ins.f32.to_f32(setup, u0)
    method = ins.RKMethods.RK44()

    def energy(u):
        st = ad.timesteps(method, ins.create_stepper(method, setup=setup, psolver=psolver, u=u), dt, nsteps, checkpoint_every=checkpoint_every)
        final.append(st.u.detach())
        return _energy(st.u, setup)

    final = []
    uu = u0.clone().requires_grad_(True)
    E = energy(uu)
    E_native = ins.total_kinetic_energy(ins.vectorfield(setup).copy_(final[0]), setup)  # the library's observer on the same field
    (grad,) = torch.autograd.grad(E, uu)
    gen = torch.Generator(device=setup.device).manual_seed(seed)
    v = ins.vectorfield(setup)
    v.copy_(torch.randn(v.shape, generator=gen, dtype=torch.float64, device=setup.device))
    v = ins.apply_bc_u(ins.project_(ins.apply_bc_u(v, 0.0, setup), setup, psolver64 if f32 else psolver, ins.scalarfield(setup)), 0.0, setup)
    v = v * (float(u0.norm()) / float(v.norm()))
    if f32:
        v = ins.f32.to_f32(setup, v)
    e = 1e-2 if f32 else 1e-4
    with torch.no_grad():
        fd = (float(energy(u0 + e * v)) - float(energy(u0 - e * v))) / (2 * e)
    dJ = float((grad.double() * v.double()).sum())
    gnorm = float(grad.norm())
    if verbose:
        print(f"E = {float(E.detach()):.9f} after {nsteps} steps; |g| = {gnorm:.6e}; <g, v> = {dJ:.9e}, central difference {fd:.9e}")
    return dict(E=float(E.detach()), E_native=E_native, grad=grad, gnorm=gnorm, dJ=dJ, fd=fd, rel=abs(fd - dJ) / abs(dJ), tol=FD_TOL32 if f32 else FD_TOL)


def _energy(u, setup):
    """`ins.total_kinetic_energy(u, setup)` in torch, so that it is differentiable: Σ_{Ip} Ω ½ Σ_α u_α² (on a periodic box the observer's average of
    the two faces of a volume sums to the same)."""
    g = setup.grid
    D = g.dimension
    ip = tuple(slice(lo, hi) for lo, hi in g.Ip)
    vol = 1.0
    for a in range(D):
        shape = [1] * D
        shape[a] = g.Ip[a][1] - g.Ip[a][0]
        vol = vol * torch.as_tensor(np.asarray(g.Δ[a], dtype=np.float64)[g.Ip[a][0]:g.Ip[a][1]], device=setup.device).reshape(shape)
    k = 0.5 * (u[ip].double() ** 2).sum(dim=-1)
    return (k * vol).sum()


if __name__ == "__main__":
    r = main(**_common.cli(dict(n=32, nsteps=8, dt=1e-3, Re=1600.0)))
    print(f"relative difference {r['rel']:.2e} (tolerance {r['tol']:.0e})")
