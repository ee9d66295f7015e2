#!/usr/bin/env python3
"""Kolmogorov flow: a periodic 2-D box driven by a steady sinusoidal body force (the setting of examples/Kolmogorov2D.jl), started from a
small random field; energy history and final spectrum.  dtype=float32 steps on the Float32 family (ins_amd.f32: the steady force rides in its
native stage loop), dtype=float64 (the default) through solve_unsteady.
    python examples/Kolmogorov2D.py n=256 tend=2 dtype=float32"""
import numpy as np

import _common  # noqa: F401
import ins_amd as ins


def main(n=128, tend=0.5, dt=1e-3, Re=2000.0, verbose=True, dtype="float64"):
    if dtype not in ("float32", "float64"):
        raise ValueError("dtype: 'float32' or 'float64'")
    axis = np.linspace(0.0, 1.0, n + 1)
    setup = ins.Setup(x=(axis, axis), Re=Re, bodyforce=lambda a, x, y, t: (a == 0) * 5 * np.sin(8 * np.pi * y) + 0 * x, issteadybodyforce=True)
    psolver = ins.psolver_spectral(setup)
    ustart = ins.random_field(setup, 0.0, A=1e-2, psolver=psolver)
    energy = []

    if dtype == "float32":  # the Float32 family: the steady force rides in its native stage loop; energy every 10 steps as below
        f32 = ins.f32
        cache = f32.ERKCache32(ins.RKMethods.RK44(), setup, f32.psolver_spectral32(setup))
        u32 = f32.to_f32(setup, ustart)
        nstep = max(1, int(round(tend / dt)))
        h = tend / nstep
        energy.append((0.0, ins.total_kinetic_energy(ustart, setup)))
        done = 0
        while done < nstep:
            k = min(10, nstep - done)
            f32.timesteps32_(cache, u32, h, k)
            done += k
            energy.append((done * h, ins.total_kinetic_energy(u32.double(), setup)))
            if verbose and done % 100 == 0:
                print(f"step {done}: t = {done * h:.3f}, E = {energy[-1][1]:.4e}")
        u, t = u32.double(), nstep * h
    else:

        def ehist(state):
            state.on(lambda s: s["n"] % 10 == 0 and energy.append((s["t"], ins.total_kinetic_energy(s["u"], setup))))
            return energy

        procs = dict(ehist=ins.processor(ehist))
        if verbose:
            procs["log"] = ins.timelogger(nupdate=100)
        (u, _, t), out = ins.solve_unsteady(setup=setup, tlims=(0.0, tend), ustart=ustart, Δt=dt, psolver=psolver, processors=procs)
    spec = ins.observespectrum(dict(u=u, temp=None, t=t, n=0), setup=setup)
    up = ins.to_numpy(ins.interpolate_u_p(u, setup))
    # the forcing drives u(y) ~ sin(8πy): its Fourier amplitude in the mean x-velocity profile
    prof = up[1:-1, 1:-1, 0].mean(axis=0)
    y = np.asarray(setup.grid.xp[1][1:-1])
    amp = 2 * np.mean(prof * np.sin(8 * np.pi * y))
    return dict(energy=energy, ehat=spec["ehat"].value, κ=spec["κ"], forced_mode=float(amp), maxdiv=ins.max_abs_divergence(u, setup), u=ins.to_numpy(u))


if __name__ == "__main__":
    r = main(**_common.cli(dict(n=128, tend=0.5, dt=1e-3, Re=2000.0, dtype="float64")))
    print(f"E: {r['energy'][0][1]:.3e} -> {r['energy'][-1][1]:.3e}; amplitude of the forced mode in <u>(y): {r['forced_mode']:.4f}; max|div u| = {r['maxdiv']:.2e}")
