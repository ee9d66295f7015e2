#!/usr/bin/env python3
"""Rayleigh-Bénard convection in a 3-D box (the setting of examples/RayleighBenard3D.jl, which runs T = Float32): periodic in x, insulated no-slip side
walls in y, a hot bottom plate (T = 1) and a cold top plate (T = 0) in z; temperature equation with viscous heating, buoyancy in z, tanh-stretched y and z,
the direct pressure solver, RK33C2 with a fixed Δt.  dtype=float32 steps on the Float32 family (ins_amd.f32), dtype=float64 through solve_unsteady.
    python examples/RayleighBenard3D.py n=60 tend=10 dt=1e-2 dtype=float32"""
import numpy as np

import _common  # noqa: F401
import ins_amd as ins


def main(n=60, tend=10.0, dt=1e-2, dtype="float32", verbose=True):
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype: 'float32' or 'float64'")
    temperature = ins.temperature_equation(
        Pr=0.71, Ra=1e7, Ge=1.0, dodissipation=True, gdir=2, nondim_type=1,
        boundary_conditions=((ins.PeriodicBC(), ins.PeriodicBC()), (ins.SymmetricBC(), ins.SymmetricBC()), (ins.DirichletBC(1.0), ins.DirichletBC(0.0))))
    x = (np.linspace(0.0, np.pi, 2 * n), ins.tanh_grid(0.0, 1.0, n, 1.2), ins.tanh_grid(0.0, 1.0, n, 1.2))  # LinRange(0, π, 2n): 2n points
    walls = (ins.DirichletBC(), ins.DirichletBC())
    setup = ins.Setup(x=x, boundary_conditions=((ins.PeriodicBC(), ins.PeriodicBC()), walls, walls), temperature=temperature)  # Re = 1/α1
    psolver = ins.psolver_direct(setup)
    method = ins.RKMethods.RK33C2()
    ufunc = lambda a, x, y, z: 0 * (x + y + z)  # noqa: E731
    tempfunc = lambda x, y, z: 0.5 + np.sin(20 * x) * np.sin(20 * np.pi * y) / 100 + 0 * z  # noqa: E731
    ustart = ins.velocityfield(setup, ufunc, psolver=psolver)
    g = setup.grid
    nsteps = int(round(tend / dt))
    if dtype == "float32":
        f32 = ins.f32
        ps32 = f32.psolver_wrap32(setup, psolver)
        cache = f32.ERKCache32(method, setup, ps32)
        u = f32.to_f32(setup, ustart)
        temp = f32.temperaturefield32(setup, tempfunc)
        done = 0
        while done < nsteps:
            k = min(100, nsteps - done)
            f32.timesteps32_(cache, u, dt, k, temp=temp)
            done += k
            if verbose:
                print(f"step {done}: t = {done * dt:.2f}, max|u| = {float(u.abs().max()):.3e}")
        maxdiv = f32.max_abs_divergence32(u, setup, ps32)
        T, U = temp.cpu().numpy(), u.cpu().numpy()
    else:
        tempstart = ins.temperaturefield(setup, tempfunc)
        procs = dict(log=ins.timelogger(nupdate=100)) if verbose else {}
        (u, temp, t), _ = ins.solve_unsteady(setup=setup, tlims=(0.0, nsteps * dt), ustart=ustart, tempstart=tempstart, method=method, Δt=dt,
                                             psolver=psolver, processors=procs)
        maxdiv = ins.max_abs_divergence(u, setup)
        T, U = ins.to_numpy(temp), ins.to_numpy(u)
    # Nusselt numbers: the heat flux -∂T/∂z through the two plates, summed over the plate with the face areas
    T64 = T.astype(np.float64)
    dz1, dz2 = g.Δu[2][0], g.Δu[2][-2]
    area = np.multiply.outer(np.asarray(g.Δ[0]), np.asarray(g.Δ[1]))
    lo = float(np.sum((-(T64[:, :, 1] - T64[:, :, 0]) / dz1 * area)[1:-1, 1:-1]))
    hi = float(np.sum((-(T64[:, :, -2] - T64[:, :, -3]) / dz2 * area)[1:-1, 1:-1]))
    inner = T64[1:-1, 1:-1, 1:-1]
    hmin = min(float(np.min(np.asarray(g.Δ[a])[1:-1])) for a in range(3))
    return dict(temp=T, u=U, nusselt=(lo, hi), Tmin=float(inner.min()), Tmax=float(inner.max()), maxdiv=float(maxdiv), hmin=hmin,
                umax=float(np.max(np.abs(U))), Re=setup.Re)


if __name__ == "__main__":
    r = main(**_common.cli(dict(n=60, tend=10.0, dt=1e-2, dtype="float32")))
    lo, hi = r["nusselt"]
    print(f"Re = {r['Re']:.1f}: Nu(bottom) = {lo:.3f}, Nu(top) = {hi:.3f}; T in [{r['Tmin']:.3f}, {r['Tmax']:.3f}]; max|u| = {r['umax']:.3e}; "
          f"max|div u| = {r['maxdiv']:.3e}")
